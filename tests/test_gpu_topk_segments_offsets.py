"""The segmented partial sort with its table of borders on the device (rdst_hip_topk_segments_device_offsets).
Every case compares the WHOLE output buffers — guard bands, rows, and the slots from k_s on, all pre-filled — bit for bit with
the numpy statement (topk_segments_inputs.expected_rows: per segment the first k_s of a stable argsort by the mapped key) and
with what rdst_hip_topk_segments_device writes into equally pre-filled buffers for the same table given from the host, and
checks that the input is unchanged, that nothing was written before or behind the scratch the call was told about, and that
the device error word is clean.  Plans are compared item for item with topk_segments_inputs.plan and the host plan."""
import re

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
ERR_ARG, ERR_DEVICE = -1, -5
TABLE_BIT = 16
UNBOUNDED = (1 << 32) - 1
WIDTH_PAIRS = (("uint8", 0), ("uint16", 0), ("uint32", 0), ("uint64", 0), ("u128", 0), ("uint32", 4), ("float32", 8), ("int64", 4), ("float64", 8))


def _torch_index(ib):
    import torch
    return {None: None, 0: None, 4: torch.int32, 8: torch.int64}[ib]


def _torch_offsets(off, ob):
    import torch
    return torch.from_numpy(np.asarray(off).astype(np.int64)).to(torch.int32 if ob == 4 else torch.int64).cuda()


class Table:
    """keys and the table of borders on the device (both widths), with what does not depend on k computed once"""

    def __init__(self, a, off, key=None):
        self.a, self.off, self.key = np.ascontiguousarray(a), np.asarray(off, dtype=np.uint64), key
        self.name = key if key else a.dtype.name
        self.t = H.to_device(self.a)
        self.n = len(self.a)
        self.n_seg = len(self.off) - 1
        self.longest = int((self.off[1:] - self.off[:-1]).max())
        self.toff = {ob: _torch_offsets(self.off, ob) for ob in (4, 8)}
        self._ordered, self._want = {}, {}

    def want(self, k, largest, ib):
        """the expected bytes of the guarded key buffer and the expected guarded index buffer"""
        if (k, largest) not in self._want:
            if largest not in self._ordered:
                self._ordered[largest] = S.table_order(self.a, self.off, largest, self.key)
            per_key = 2 if T.is_wide(self.key) else 1
            want_k = np.full((self.n_seg * k + 2 * GUARD) * per_key * self.a.dtype.itemsize, FILL_KEY, dtype=np.uint8).view(self.a.dtype)
            rows_k = want_k[GUARD * per_key:(GUARD + self.n_seg * k) * per_key].reshape((self.n_seg, k, 2) if per_key == 2 else (self.n_seg, k))
            want_i = np.full(self.n_seg * k + 2 * GUARD, FILL_INDEX, dtype=np.int64)
            S.expected_rows(self.a, self.off, k, largest, self.key, rows_k, want_i[GUARD:GUARD + self.n_seg * k].reshape(self.n_seg, k), self._ordered[largest])
            self._want[(k, largest)] = (want_k.view(np.uint8).reshape(-1), want_i)
        return self._want[(k, largest)]


def _outputs(tb, k, ib):
    import torch
    per_key = 2 if T.is_wide(tb.key) else 1
    slots = tb.n_seg * k
    raw_k = torch.full(((slots + 2 * GUARD) * per_key * tb.a.dtype.itemsize,), FILL_KEY, dtype=torch.uint8, device="cuda")
    out_k = raw_k.view(tb.t.dtype)[GUARD * per_key:(GUARD + slots) * per_key]
    raw_i = out_i = None
    if ib:
        raw_i = torch.full((slots + 2 * GUARD,), FILL_INDEX, dtype=_torch_index(ib), device="cuda")
        out_i = raw_i[GUARD:GUARD + slots]
    return raw_k, out_k, raw_i, out_i


def _call(gpu, tb, k, largest=False, ib=None, ob=8, far_capacity=0, scratch=None, toff=None):
    """enqueues one call (check=False) on pre-filled, guarded outputs and a scratch of EXACTLY the stated size between two
    poisoned bands; returns what _verify needs"""
    import torch
    raw_k, out_k, raw_i, out_i = _outputs(tb, k, ib)
    need = gpu.topk_segments_device_offsets_scratch_bytes(tb.n_seg, far_capacity, k, tb.name, ib or 0)
    assert need > 0
    if scratch is not None:                                                 # shared by several calls: the bands lie round the largest need
        assert scratch.numel() >= need + 2 * SLACK
        need = scratch.numel() - 2 * SLACK
    raw_s = scratch if scratch is not None else torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    got = gpu.topk_segments_device_offsets_tensor(tb.t, tb.toff[ob] if toff is None else toff, k, largest=largest, index=_torch_index(ib),
                                                  scratch=raw_s[SLACK:SLACK + need], far_capacity=far_capacity, check=False, key=tb.key, out=(out_k, out_i))
    assert got[0] is out_k and got[1] is out_i
    return raw_k, raw_i, raw_s, need


def _host_entry(gpu, tb, k, largest, ib):
    """rdst_hip_topk_segments_device with the table from the host, into equally pre-filled buffers"""
    raw_k, out_k, raw_i, out_i = _outputs(tb, k, ib)
    gpu.topk_segments_device_tensor(tb.t, tb.off, k, largest=largest, index=_torch_index(ib), check=False, key=tb.key, out=(out_k, out_i))
    return raw_k, raw_i


def _verify(gpu, tb, k, largest, ib, bufs, what="", host=None):
    raw_k, raw_i, raw_s, need = bufs
    gpu.device_status()                                                     # the error word is clean
    what = f"{what} {tb.name} segments = {tb.n_seg} k = {k} largest = {largest} index = {ib}"
    per_key = 2 if T.is_wide(tb.key) else 1
    want_k, want_i = tb.want(k, largest, ib)
    got_k = raw_k.cpu().numpy()
    if not np.array_equal(got_k, want_k):
        bad = np.flatnonzero(got_k != want_k)
        slot = int(bad[0]) // (per_key * tb.a.dtype.itemsize) - GUARD
        raise AssertionError(f"{what}: keys differ in {len(bad)} bytes, first in row {slot // k} slot {slot % k} "
                             f"(segment of {int(tb.off[slot // k + 1] - tb.off[slot // k]) if 0 <= slot < tb.n_seg * k else '?'} keys)")
    if ib:
        got_i = raw_i.cpu().numpy().astype(np.int64)
        if not np.array_equal(got_i, want_i):
            slot = int(np.flatnonzero(got_i != want_i)[0]) - GUARD
            raise AssertionError(f"{what}: positions differ, first in row {slot // k} slot {slot % k}: {got_i[slot + GUARD]} != {want_i[slot + GUARD]}")
    if host is not None:
        assert bool((host[0] == raw_k).all()) and (not ib or bool((host[1] == raw_i).all())), what + ": differs from the host-offsets entry"
    assert np.array_equal(H.to_host(tb.t, tb.a.dtype).view(np.uint8), tb.a.view(np.uint8)), what + ": the input changed"
    assert bool((raw_s[:SLACK] == POISON).all()) and bool((raw_s[SLACK + need:] == POISON).all()), what + ": written outside the scratch"


def _untouched(tb, k, ib, bufs, what):
    """nothing was written: outputs and guards hold their fill, the input is as it was"""
    raw_k, raw_i, raw_s, need = bufs
    assert bool((raw_k == FILL_KEY).all()) and (raw_i is None or bool((raw_i == FILL_INDEX).all())), what + ": an output element was written"
    assert np.array_equal(H.to_host(tb.t, tb.a.dtype).view(np.uint8), tb.a.view(np.uint8)), what + ": the input changed"
    assert bool((raw_s[:SLACK] == POISON).all()) and bool((raw_s[SLACK + need:] == POISON).all()), what + ": written outside the scratch"


def _table_error(gpu):
    """device_status() raises RDST_ERR_DEVICE with the table bit in the word, once: the next look is clean"""
    with pytest.raises(gpu.RdstHipError) as e:
        gpu.device_status()
    assert e.value.code == ERR_DEVICE
    word = int(re.search(r"device error word = 0x([0-9a-f]+)", str(e.value)).group(1), 16)
    assert word & TABLE_BIT, hex(word)
    gpu.device_status()


@pytest.fixture
def stream_max(gpu):
    """the setter, put back to the default afterwards"""
    yield gpu.set_topk_segments_stream_max
    gpu.set_topk_segments_stream_max(0)


# ---- 1: the length table, both modes -------------------------------------------------------------------------------------------

_TABLES = {}


def _length_table(gpu, key, ib):
    """0, 1, 2, wave_max, wave_max + 1, block_max, block_max + 1 of segment_lengths, a segment of stream_max + 1 and one of
    3 * 2^17 + 5 keys; a gap before the first border and a tail behind the last"""
    if (key, bool(ib)) not in _TABLES:
        _TABLES.clear()                                                     # one table on the device at a time
        kb = T.key_bytes(key)
        wm, bm, sm, ksm = gpu.topk_segments_limits(key, ib or 0)
        assert (wm, bm, sm, ksm) == S.limits(kb, bool(ib))
        lengths = [n for n in S.segment_lengths(wm, bm) if n in (0, 1, 2, wm, wm + 1, bm, bm + 1)]
        assert len(lengths) == 7
        lengths = lengths[:4] + [sm + 1] + lengths[4:] + [3 * (1 << 17) + 5]
        off = np.cumsum([3] + lengths).astype(np.uint64)
        _TABLES[(key, bool(ib))] = Table(S.keys_for(int(off[-1]) + 2, key, 11 + kb), off, key if T.is_wide(key) else None)
    tb = _TABLES[(key, bool(ib))]
    return (tb,) + tuple(gpu.topk_segments_limits(key, ib or 0))


def _async_length_table(gpu, key, ib):
    tb, wm, bm, sm, ksm = _length_table(gpu, key, ib)
    for i, k in enumerate(k for k in S.table_ks(wm, bm) if k <= ksm):
        for largest in (False, True):
            host = _host_entry(gpu, tb, k, largest, ib)
            for ob in (4, 8):
                _verify(gpu, tb, k, largest, ib, _call(gpu, tb, k, largest, ib, ob), f"async, {ob}-byte offsets", host)


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_length_table_async_keys_only(gpu, key, kb):
    _async_length_table(gpu, key, None)


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_length_table_async_with_an_index(gpu, key, ib):
    _async_length_table(gpu, key, ib)


def _wait_length_table(gpu, stream_max, key, ib):
    """the border lowered to 3 block_max: stream_max + 1 and 3 * 2^17 + 5 go far, nothing is of the stream class but for the
    segment of block_max + 1 keys; k = block_max + 1 sends that one far too"""
    tb, wm, bm, _sm, ksm = _length_table(gpu, key, ib)
    stream_max(3 * bm)
    kb = T.key_bytes(key)
    for k in (1, 65, bm, bm + 1):
        counts = S.plan(tb.off, k, kb, bool(ib), 3 * bm)[1]
        assert counts == ((3, 2, 1, 2) if k <= ksm else (3, 2, 0, 3))
        for largest in (False, True):
            host = _host_entry(gpu, tb, k, largest, ib)
            ob = 4 if largest else 8
            _verify(gpu, tb, k, largest, ib, _call(gpu, tb, k, largest, ib, ob, far_capacity=tb.n), f"wait, {ob}-byte offsets", host)


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_length_table_wait_keys_only(gpu, stream_max, key, kb):
    _wait_length_table(gpu, stream_max, key, None)


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_length_table_wait_with_an_index(gpu, stream_max, key, ib):
    _wait_length_table(gpu, stream_max, key, ib)


# ---- 2: the device plan against the host plan ----------------------------------------------------------------------------------

@pytest.mark.parametrize("key,ib", WIDTH_PAIRS, ids=[f"{k}-i{8 * ib}" for k, ib in WIDTH_PAIRS])
def test_device_plan_is_the_host_plan_item_for_item(gpu, stream_max, key, ib):
    kb = T.key_bytes(key)
    wm, bm, sm, ksm = gpu.topk_segments_limits(key, ib)
    rng = np.random.default_rng(5 + kb + ib)
    lengths = [0, 1, 2, wm, wm + 1, bm, bm + 1, bm + 1, 2 * bm + 3, 3 * bm, 3 * bm + 1, sm, sm + 1, sm + 1, wm, bm, 0, 1, bm - 1, bm - 1, 600, 600, 4 * bm + 7]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    off = np.cumsum([3] + lengths).astype(np.uint64)
    n = int(off[-1]) + 9
    for border in (0, 3 * bm):
        stream_max(border)
        for k in (1, bm, bm + 1):
            for ob in (4, 8):
                toff = _torch_offsets(off, ob)
                for unbounded in (False, True):
                    want = S.plan(off, k, kb, bool(ib), UNBOUNDED if unbounded else border)
                    got = gpu.topk_segments_plan_device(toff, n, k, key, ib, unbounded_stream=unbounded)
                    assert got[3] == 0
                    assert got[:3] == want, f"{key} index = {ib} k = {k} border = {border} unbounded = {unbounded}"
                    if not unbounded:
                        assert got[:3] == gpu.topk_segments_plan(off, n, k, key, ib)
                    elif k <= ksm:                                          # beyond the default stream_max, and of the stream class
                        assert got[1][3] == 0 and got[2] == 0
                        assert sum(1 for start, ln, seg in got[0][got[1][0] + got[1][1]:] if ln > S.STREAM_MAX_DEFAULT) == 2
                    else:
                        assert got[1][2] == 0 and got[1][3] == sum(1 for ln in lengths if ln > bm)
    gpu.device_status()                                                     # the hook leaves the error word alone


def test_plan_hook_reports_invalid_tables_as_flags(gpu):
    off = np.cumsum([0, 5, 700, 0, 9]).astype(np.int64)
    dec = off.copy()
    dec[2] = off[3] + 1
    for ob in (4, 8):
        assert gpu.topk_segments_plan_device(_torch_offsets(dec, ob), 800, 3, "uint32")[3] & 1
        assert gpu.topk_segments_plan_device(_torch_offsets(off, ob), int(off[-1]) - 1, 3, "uint32")[3] == 2
        assert gpu.topk_segments_plan_device(_torch_offsets(off, ob), int(off[-1]), 3, "uint32")[3] == 0
    gpu.device_status()


# ---- 3: counted grids ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,ib", (("uint32", 4), ("uint64", None), ("uint16", None)))
def test_surplus_waves_and_workgroups_return(gpu, key, ib):
    """a few thousand segments, almost all empty, a handful in each class: the grids are bounds, the counts stand in the header"""
    wm, bm, _sm, _ksm = gpu.topk_segments_limits(key, ib or 0)
    lengths = np.zeros(5000, dtype=np.int64)
    at = np.random.default_rng(2).choice(5000, size=14, replace=False)
    lengths[at] = [1, 2, 3, wm, 77, wm + 1, 1025, bm, bm - 1, bm + 1, 2 * bm + 3, 3 * bm + 1, wm + 9, 5]
    off = np.concatenate([[1], 1 + np.cumsum(lengths)]).astype(np.uint64)
    tb = Table(S.keys_for(int(off[-1]) + 3, key, 9), off)
    assert S.plan(off, 7, T.key_bytes(key), bool(ib), UNBOUNDED)[1] == (6, 5, 3, 0)
    for k, largest, ob in ((7, False, 4), (bm, True, 8)):
        _verify(gpu, tb, k, largest, ib, _call(gpu, tb, k, largest, ib, ob), "sparse table", _host_entry(gpu, tb, k, largest, ib))


def test_counts_that_meet_the_grid_bounds(gpu):
    """every segment one key: the wave class's count is min(n_segments, len); every segment wave_max + 1 keys: the block
    class's is len / (wave_max + 1)"""
    wm = gpu.topk_segments_limits("uint32", 0)[0]
    ones = Table(T.three_values(1031, "uint32", 4), np.arange(1032, dtype=np.uint64))
    assert S.plan(ones.off, 2, 4, False, UNBOUNDED)[1] == (1031, 0, 0, 0)
    _verify(gpu, ones, 2, False, None, _call(gpu, ones, 2, False, None, 4), "segments of one key")
    _verify(gpu, ones, 1, True, 8, _call(gpu, ones, 1, True, 8, 8), "segments of one key")
    blocks = Table(S.keys_for(37 * (wm + 1), "uint32", 6), np.arange(38, dtype=np.uint64) * np.uint64(wm + 1))
    assert S.plan(blocks.off, 5, 4, True, UNBOUNDED)[1] == (0, 37, 0, 0)
    _verify(gpu, blocks, 5, True, 4, _call(gpu, blocks, 5, True, 4, 8), "segments of wave_max + 1 keys")
    _verify(gpu, blocks, wm + 1, False, None, _call(gpu, blocks, wm + 1, False, None, 4), "segments of wave_max + 1 keys")


# ---- 4: what the device refuses -------------------------------------------------------------------------------------------------------

def _small_table(gpu, key="uint32", ib=None, extra=()):
    bm = gpu.topk_segments_limits(key, ib or 0)[1]
    off = np.cumsum([2, 5, 700, 0, bm, 9] + list(extra)).astype(np.uint64)
    return Table(S.keys_for(int(off[-1]) + 4, key, 13), off), bm


def _invalid_tables(tb):
    """(name, offsets, len): a decreasing pair, a last offset past len"""
    dec = tb.off.astype(np.int64)
    dec[2] = dec[3] + 1
    yield "a decreasing pair", dec, tb.n
    yield "a last offset of len + 1", tb.off, int(tb.off[-1]) - 1


@pytest.mark.parametrize("ob", [4, 8])
def test_invalid_tables(gpu, ob):
    import torch
    tb, _bm = _small_table(gpu, "float32", 4)
    gpu.device_status()
    for name, bad, bad_n in _invalid_tables(tb):
        short = Table(tb.a[:bad_n], tb.off, None)                           # (the borders of the result rows; the call gets `bad`)
        toff = _torch_offsets(bad, ob)
        # asynchronous: nothing written, RDST_ERR_DEVICE once
        bufs = _call(gpu, short, 3, False, 4, ob, toff=toff)
        _table_error(gpu)
        _untouched(short, 3, 4, bufs, "async, " + name)
        # wait mode: the return code says so, nothing written, the error word clean
        raw_k, out_k, raw_i, out_i = _outputs(short, 3, 4)
        need = gpu.topk_segments_device_offsets_scratch_bytes(short.n_seg, short.n, 3, "float32", 4)
        raw_s = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
        with pytest.raises(gpu.RdstHipError) as e:
            gpu.topk_segments_device_offsets_tensor(short.t, toff, 3, index=torch.int32, scratch=raw_s[SLACK:SLACK + need], far_capacity=short.n, check=False,
                                                    out=(out_k, out_i))
        assert e.value.code == ERR_ARG and ("non-decreasing" in str(e.value) or "past len" in str(e.value))
        gpu.device_status()
        _untouched(short, 3, 4, (raw_k, raw_i, raw_s, need), "wait, " + name)


def test_a_k_the_async_mode_cannot_answer(gpu):
    """k > k_stream_max and one segment of block_max + 1 keys: nothing written, bit 0x10; the wait mode serves it"""
    bm = gpu.topk_segments_limits("uint32", 0)[1]
    tb = _small_table(gpu, "uint32", None, extra=(bm + 1, 3))[0]
    gpu.device_status()
    bufs = _call(gpu, tb, bm + 1, False, None, 8)
    _table_error(gpu)
    _untouched(tb, bm + 1, None, bufs, "k = block_max + 1 without far_capacity")
    _verify(gpu, tb, bm, False, None, _call(gpu, tb, bm, False, None, 8), "k = block_max")
    _verify(gpu, tb, bm + 1, False, None, _call(gpu, tb, bm + 1, False, None, 8, far_capacity=bm + 1), "far_capacity = the longest")


def test_far_capacity_below_the_longest_far_segment(gpu, stream_max):
    import torch
    bm = gpu.topk_segments_limits("uint64", 8)[1]
    tb = _small_table(gpu, "uint64", 8, extra=(2 * bm + 3,))[0]
    stream_max(bm)
    longest = tb.longest
    assert longest == 2 * bm + 3 and S.plan(tb.off, 4, 8, True, bm)[2] == longest
    raw_k, out_k, raw_i, out_i = _outputs(tb, 4, 8)
    need = gpu.topk_segments_device_offsets_scratch_bytes(tb.n_seg, longest - 1, 4, "uint64", 8)
    raw_s = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu.RdstHipError) as e:
        gpu.topk_segments_device_offsets_tensor(tb.t, tb.toff[8], 4, index=torch.int64, scratch=raw_s[SLACK:SLACK + need], far_capacity=longest - 1,
                                                check=False, out=(out_k, out_i))
    assert e.value.code == ERR_ARG and "far_capacity" in str(e.value)
    gpu.device_status()
    _untouched(tb, 4, 8, (raw_k, raw_i, raw_s, need), "far_capacity = longest - 1")
    _verify(gpu, tb, 4, False, 8, _call(gpu, tb, 4, False, 8, 4, far_capacity=longest), "far_capacity = longest")


# ---- 5: stream order, scratch reuse ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stream", ["default", "other"])
def test_offsets_from_a_cumsum_behind_a_kernel_that_writes_the_keys(gpu, stream):
    import torch
    wm, bm, _sm, _ksm = gpu.topk_segments_limits("uint32", 4)
    rng = np.random.default_rng(51)
    lengths = rng.integers(0, 41, size=2001)
    lengths[rng.choice(2001, size=8, replace=False)] = [wm, wm + 1, 600, bm, bm + 1, 2 * bm + 3, 0, 1]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    a = S.keys_for(int(off[-1]) + 5, "uint32", 23)
    tb = Table(np.zeros_like(a), off)
    src = H.to_device(a).view(torch.int32) ^ 0x5A5A5A5A
    tlen = torch.from_numpy(lengths).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if stream == "other" else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        for _ in range(4):                                                  # work in front of the write, so that the call is enqueued behind it
            src = (src ^ 0x1111) ^ 0x1111
        tb.t.view(torch.int32).copy_(src ^ 0x5A5A5A5A)
        toff = torch.zeros(len(lengths) + 1, dtype=torch.int64, device="cuda")
        toff[1:] = torch.cumsum(tlen, 0)                                    # queued on the stream; nothing comes to the host
        bufs = _call(gpu, tb, 9, True, 4, toff=toff)
        bufs32 = _call(gpu, tb, 3, False, 4, toff=toff.to(torch.int32))
    torch.cuda.synchronize()
    tb.a = a                                                                # (what the producer wrote)
    _verify(gpu, tb, 9, True, 4, bufs, f"cumsum, {stream} stream")
    _verify(gpu, tb, 3, False, 4, bufs32, f"cumsum, {stream} stream, int32")


def test_two_calls_back_to_back_on_one_scratch(gpu, stream_max):
    import torch
    bm = gpu.topk_segments_limits("uint64", 0)[1]
    stream_max(2 * bm)
    off1 = np.cumsum([1, 3, 700, bm + 9, 3 * bm + 1]).astype(np.uint64)
    off2 = np.cumsum([5, 2 * bm + 3, 1, 513, bm + 1, 0, 7]).astype(np.uint64)
    t1, t2 = Table(S.keys_for(int(off1[-1]) + 1, "uint64", 1), off1), Table(S.keys_for(int(off2[-1]), "uint64", 2), off2)
    need = max(gpu.topk_segments_device_offsets_scratch_bytes(t1.n_seg, t1.n, bm + 1, "uint64"), gpu.topk_segments_device_offsets_scratch_bytes(t2.n_seg, 0, 40, "uint64"))
    scratch = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    b1 = _call(gpu, t1, bm + 1, False, None, 8, far_capacity=t1.n, scratch=scratch)    # far segments, whose scratch lies behind the plan
    b2 = _call(gpu, t2, 40, True, None, 4, scratch=scratch)
    b3 = _call(gpu, t1, 40, True, None, 8, scratch=scratch)
    b4 = _call(gpu, t2, 2, False, None, 8, far_capacity=t2.n, scratch=scratch)
    _verify(gpu, t1, bm + 1, False, None, b1, "first of four")
    _verify(gpu, t2, 40, True, None, b2, "second of four")
    _verify(gpu, t1, 40, True, None, b3, "third of four")
    _verify(gpu, t2, 2, False, None, b4, "fourth of four")
