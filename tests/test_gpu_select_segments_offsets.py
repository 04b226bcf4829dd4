"""The segmented select with its table of borders on the device (rdst_hip_select_segments_device_offsets).
Every case compares the WHOLE output buffers — guard bands, rows, and the slots without a rank, all pre-filled — bit for bit
with the numpy statement (select_segments_inputs.expected_rows: per segment the element of a stable argsort by the mapped key
at the rank the spec stands for) and with what rdst_hip_select_segments_device writes into equally pre-filled buffers for the
same table given from the host, and checks that the input is unchanged, that nothing was written before or behind the scratch
the call was told about, and that the device error word is clean.  Every table is valid or refused by the plan."""
import re

import numpy as np
import pytest

import helpers as H
import select_segments_inputs as Q
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


def _operands(specs):
    """the wrapper's two lists and its method for a list of specs: absolute ranks first, one mode (the tables here keep them so)"""
    assert [s for s in specs if s[1] == 0] + [s for s in specs if s[1] != 0] == list(specs)
    modes = {s[2] for s in specs if s[1] != 0}
    assert len(modes) <= 1
    return [s[0] for s in specs if s[1] == 0], [(s[0], s[1]) for s in specs if s[1] != 0], {0: "lower", 1: "higher", 2: "nearest"}[modes.pop() if modes else 0]


def _absolute(ranks):
    return [(int(r), 0, 0) for r in ranks]


class Table:
    """keys and the table of borders on the device (both widths), with what does not depend on the specs computed once"""

    def __init__(self, a, off, key=None):
        self.a, self.off, self.key = np.ascontiguousarray(a), np.asarray(off, dtype=np.uint64), key
        self.name = key if key else a.dtype.name
        self.t = H.to_device(self.a)
        self.n = len(self.a)
        self.n_seg = len(self.off) - 1
        self.longest = int((self.off[1:] - self.off[:-1]).max())
        self.toff = {ob: _torch_offsets(self.off, ob) for ob in (4, 8)}
        self._ordered, self._want = {}, {}

    def want(self, specs, largest):
        """the expected bytes of the guarded key buffer and the expected guarded index buffer"""
        at = (tuple(map(tuple, specs)), largest)
        if at not in self._want:
            if largest not in self._ordered:
                self._ordered[largest] = S.table_order(self.a, self.off, largest, self.key)
            per_key, nr = 2 if T.is_wide(self.key) else 1, len(specs)
            want_k = np.full((self.n_seg * nr + 2 * GUARD) * per_key * self.a.dtype.itemsize, FILL_KEY, dtype=np.uint8).view(self.a.dtype)
            rows_k = want_k[GUARD * per_key:(GUARD + self.n_seg * nr) * per_key].reshape((self.n_seg, nr, 2) if per_key == 2 else (self.n_seg, nr))
            want_i = np.full(self.n_seg * nr + 2 * GUARD, FILL_INDEX, dtype=np.int64)
            Q.expected_rows(self.a, self.off, specs, largest, self.key, rows_k, want_i[GUARD:GUARD + self.n_seg * nr].reshape(self.n_seg, nr),
                            self._ordered[largest])
            self._want = {at: (want_k.view(np.uint8).reshape(-1), want_i)}          # the latest only: the callers go set by set
        return self._want[at]


def _outputs(tb, nr, ib):
    import torch
    per_key = 2 if T.is_wide(tb.key) else 1
    slots = tb.n_seg * nr
    raw_k = torch.full(((slots + 2 * GUARD) * per_key * tb.a.dtype.itemsize,), FILL_KEY, dtype=torch.uint8, device="cuda")
    out_k = raw_k.view(tb.t.dtype)[GUARD * per_key:(GUARD + slots) * per_key]
    raw_i = out_i = None
    if ib:
        raw_i = torch.full((slots + 2 * GUARD,), FILL_INDEX, dtype=_torch_index(ib), device="cuda")
        out_i = raw_i[GUARD:GUARD + slots]
    return raw_k, out_k, raw_i, out_i


def _call(gpu, tb, specs, largest=False, ib=None, ob=8, far_capacity=0, scratch=None, toff=None):
    """enqueues one call (check=False) on pre-filled, guarded outputs and a scratch of EXACTLY the stated size between two
    poisoned bands; returns what _verify needs"""
    import torch
    raw_k, out_k, raw_i, out_i = _outputs(tb, len(specs), ib)
    need = gpu.select_segments_device_offsets_scratch_bytes(tb.n_seg, far_capacity, len(specs), tb.name, ib or 0)
    assert need > 0
    if scratch is not None:                                                 # shared by several calls: the bands lie round the largest need
        assert scratch.numel() >= need + 2 * SLACK
        need = scratch.numel() - 2 * SLACK
    raw_s = scratch if scratch is not None else torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    ranks, quantiles, method = _operands(specs)
    got = gpu.select_segments_device_offsets_tensor(tb.t, tb.toff[ob] if toff is None else toff, ranks=ranks, quantiles=quantiles, method=method,
                                                    largest=largest, index=_torch_index(ib), scratch=raw_s[SLACK:SLACK + need], far_capacity=far_capacity,
                                                    check=False, key=tb.key, out=(out_k, out_i))
    assert got[0] is out_k and got[1] is out_i
    return raw_k, raw_i, raw_s, need


def _host_entry(gpu, tb, specs, largest, ib):
    """rdst_hip_select_segments_device with the table from the host, into equally pre-filled buffers"""
    raw_k, out_k, raw_i, out_i = _outputs(tb, len(specs), ib)
    ranks, quantiles, method = _operands(specs)
    gpu.select_segments_device_tensor(tb.t, tb.off, ranks=ranks, quantiles=quantiles, method=method, largest=largest, index=_torch_index(ib), check=False,
                                      key=tb.key, out=(out_k, out_i))
    return raw_k, raw_i


def _verify(gpu, tb, specs, largest, ib, bufs, what="", host=None):
    raw_k, raw_i, raw_s, need = bufs
    gpu.device_status()                                                     # the error word is clean
    nr = len(specs)
    what = f"{what} {tb.name} segments = {tb.n_seg} specs = {list(specs)[:6]} largest = {largest} index = {ib}"
    per_key = 2 if T.is_wide(tb.key) else 1
    want_k, want_i = tb.want(specs, largest)
    got_k = raw_k.cpu().numpy()
    if not np.array_equal(got_k, want_k):
        bad = np.flatnonzero(got_k != want_k)
        slot = int(bad[0]) // (per_key * tb.a.dtype.itemsize) - GUARD
        raise AssertionError(f"{what}: keys differ in {len(bad)} bytes, first in row {slot // nr} slot {slot % nr} "
                             f"(segment of {int(tb.off[slot // nr + 1] - tb.off[slot // nr]) if 0 <= slot < tb.n_seg * nr else '?'} keys)")
    if ib:
        got_i = raw_i.cpu().numpy().astype(np.int64)
        if not np.array_equal(got_i, want_i):
            slot = int(np.flatnonzero(got_i != want_i)[0]) - GUARD
            raise AssertionError(f"{what}: positions differ, first in row {slot // nr} slot {slot % nr}: {got_i[slot + GUARD]} != {want_i[slot + GUARD]}")
    if host is not None:
        assert bool((host[0] == raw_k).all()) and (not ib or bool((host[1] == raw_i).all())), what + ": differs from the host-offsets entry"
    assert np.array_equal(H.to_host(tb.t, tb.a.dtype).view(np.uint8), tb.a.view(np.uint8)), what + ": the input changed"
    assert bool((raw_s[:SLACK] == POISON).all()) and bool((raw_s[SLACK + need:] == POISON).all()), what + ": written outside the scratch"
    return want_i


def _untouched(tb, bufs, what):
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
    """0, 1, 2, wave_max, wave_max + 1, block_max, block_max + 1, and the two lengths round the border the wait-mode tests
    lower stream_max to (block_max + 1000), each at a start of every residue modulo the 16-byte vector, filler segments between"""
    if (key, bool(ib)) not in _TABLES:
        _TABLES.clear()                                                     # one table on the device at a time
        kb = T.key_bytes(key)
        wm, bm, sm, mr = gpu.select_segments_limits(key, ib or 0)
        assert (wm, bm, sm, mr) == Q.limits(kb, bool(ib))
        off, n = S.residue_table([0, 1, 2, wm, wm + 1, bm, bm + 1, bm + 1000, bm + 1001], kb)
        _TABLES[(key, bool(ib))] = Table(S.keys_for(n, key, 11 + kb), off, key if T.is_wide(key) else None)
    return _TABLES[(key, bool(ib))], gpu.select_segments_limits(key, ib or 0)[0], gpu.select_segments_limits(key, ib or 0)[1]


def _rank_sets(wm):
    """the median in all three modes, select_segments_inputs.rank_sets — the last of them with the absolute rank wave_max, which
    the short segments lack"""
    return [[Q.median(Q.LOWER)], [Q.median(Q.HIGHER)], [Q.median(Q.NEAREST)]] + Q.rank_sets(wm)


def _lacking_slots_keep_the_fill(tb, wm, want_i):
    lens = tb.off[1:] - tb.off[:-1]
    rows = want_i[GUARD:-GUARD].reshape(tb.n_seg, -1)
    short = np.flatnonzero(lens <= wm)
    assert len(short) and bool((rows[short, 0] == FILL_INDEX).all()) and bool((rows[np.flatnonzero(lens > wm), 0] != FILL_INDEX).all())


def _async_length_table(gpu, key, ib):
    tb, wm, _bm = _length_table(gpu, key, ib)
    for i, specs in enumerate(_rank_sets(wm)):
        for largest in (False, True):
            host = _host_entry(gpu, tb, specs, largest, ib)
            ob = 4 if (i + largest) % 2 else 8
            want_i = _verify(gpu, tb, specs, largest, ib, _call(gpu, tb, specs, largest, ib, ob), f"async, {ob}-byte offsets", host)
    _lacking_slots_keep_the_fill(tb, wm, want_i)


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_length_table_async_keys_only(gpu, key, kb):
    _async_length_table(gpu, key, None)


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_length_table_async_with_an_index(gpu, key, ib):
    _async_length_table(gpu, key, ib)


def _wait_length_table(gpu, stream_max, key, ib):
    """the border lowered to block_max + 1000: the segments of block_max + 1 and stream_max keys are of the stream class, those
    of stream_max + 1 keys go far"""
    tb, wm, bm = _length_table(gpu, key, ib)
    stream_max(bm + 1000)
    vec = 16 // T.key_bytes(key)
    counts = gpu.topk_segments_plan(tb.off, tb.n, 1, key, ib or 0)[1]
    assert counts[2] == 2 * vec and counts[3] == vec
    for i, specs in enumerate(_rank_sets(wm)):
        for largest in (False, True):
            host = _host_entry(gpu, tb, specs, largest, ib)
            ob = 8 if (i + largest) % 2 else 4
            want_i = _verify(gpu, tb, specs, largest, ib, _call(gpu, tb, specs, largest, ib, ob, far_capacity=tb.n), f"wait, {ob}-byte offsets", host)
    _lacking_slots_keep_the_fill(tb, wm, want_i)


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_length_table_wait_keys_only(gpu, stream_max, key, kb):
    _wait_length_table(gpu, stream_max, key, None)


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_length_table_wait_with_an_index(gpu, stream_max, key, ib):
    _wait_length_table(gpu, stream_max, key, ib)


# ---- 2: the asynchronous mode beyond the default border ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 8), ("uint64", None)))
def test_async_beyond_the_default_stream_max(gpu, dtype, ib):
    """segments of 2^17 + 1 and 3 * 2^17 + 5 keys beside short ones: one workgroup each in the asynchronous mode, the far class
    in the wait mode, the same bits.  The first holds, after one level, a tile and one key on the rank's prefix (floats: runs of
    zeros and NaNs on the ranks), the second is all equal: the stream body's depth and window paths at these lengths"""
    wm, bm, sm, _mr = gpu.select_segments_limits(dtype, ib or 0)
    n1, n2 = (1 << 17) + 1, 3 * (1 << 17) + 5
    assert sm == 1 << 17
    if np.dtype(dtype).kind == "f":
        first, ranks = Q.float_zero_nan_segment(dtype, n1, 9)
    else:
        first, r = Q.prefix_border(dtype, bm, n1, 1, 6)
        levels, c_below, m = Q.stream_select(first, r, False, bm)
        assert levels == 2 and c_below + m > bm
        ranks = [c_below, r, c_below + m - 1]
    one = T.random_keys(1, dtype, 9)
    short = S.keys_for(3 + 700 + wm + bm + 1, dtype, 4)
    a = np.concatenate([short[:3], first, short[3:703], np.repeat(one, n2), short[703:], one])
    off = np.cumsum([3, n1, 700, 0, n2, wm, bm + 1]).astype(np.uint64)
    tb = Table(a, off)
    windows = Q.window_ranks(bm) + [n2 - 1, n2 - bm - 2, 2 * (1 << 17) + 3]                # (the first segment lacks the last three)
    assert gpu.topk_segments_plan(off, tb.n, 1, dtype, ib or 0)[1] == (1, 1, 1, 2)
    for specs in (_absolute(ranks + windows), _absolute([0, n1 - 1]) + [(1, 2, 2), (1, 10, 2), (1, 1, 2)]):
        for largest in (False, True):
            host = _host_entry(gpu, tb, specs, largest, ib)
            b_async = _call(gpu, tb, specs, largest, ib, 4 if largest else 8)
            b_wait = _call(gpu, tb, specs, largest, ib, 8 if largest else 4, far_capacity=tb.n)
            _verify(gpu, tb, specs, largest, ib, b_async, "async beyond stream_max", host)
            _verify(gpu, tb, specs, largest, ib, b_wait, "wait, far_capacity = len", host)
            assert bool((b_async[0] == b_wait[0]).all()) and (not ib or bool((b_async[1] == b_wait[1]).all()))


# ---- 3: the device plan against the host plan ----------------------------------------------------------------------------------

@pytest.mark.parametrize("key,ib", WIDTH_PAIRS, ids=[f"{k}-i{8 * ib}" for k, ib in WIDTH_PAIRS])
def test_device_plan_with_k_1_is_the_host_plan_item_for_item(gpu, stream_max, key, ib):
    """rdst_hip_debug_topk_segments_plan_device with k = 1 is this entry's plan: against rdst_topk_segments_plan with the same
    border, and with the border at 2^32 - 1 for the asynchronous mode's classes"""
    kb = T.key_bytes(key)
    wm, bm, sm, _mr = gpu.select_segments_limits(key, ib)
    rng = np.random.default_rng(9 + kb + ib)
    lengths = [0, 1, 2, wm, wm + 1, bm, bm + 1, bm + 1, 2 * bm + 3, 3 * bm, 3 * bm + 1, sm, sm + 1, sm + 1, wm, bm, 0, 1, bm - 1, bm - 1, 600, 600, 4 * bm + 7]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    off = np.cumsum([3] + lengths).astype(np.uint64)
    n = int(off[-1]) + 9
    for border in (0, bm + 1000):
        for unbounded in (False, True):
            stream_max(UNBOUNDED if unbounded else border)
            want = gpu.topk_segments_plan(off, n, 1, key, ib)
            assert want == S.plan(off, 1, kb, bool(ib), UNBOUNDED if unbounded else border)
            stream_max(border)
            for ob in (4, 8):
                got = gpu.topk_segments_plan_device(_torch_offsets(off, ob), n, 1, key, ib, unbounded_stream=unbounded)
                assert got[3] == 0 and got[:3] == want, f"{key} index = {ib} border = {border} unbounded = {unbounded}"
            if unbounded:
                assert want[1][3] == 0 and want[2] == 0
    gpu.device_status()                                                     # the hook leaves the error word alone


# ---- 4: counted grids ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,ib", (("uint32", 4), ("uint64", None), ("uint16", None)))
def test_surplus_waves_and_workgroups_return(gpu, key, ib):
    """only wave-class segments in an array long enough for non-zero block and stream grid bounds, then only block-class
    segments: the grids are bounds, the counts stand in the header, and the surplus returns before any barrier"""
    kb = T.key_bytes(key)
    wm, bm, _sm, _mr = gpu.select_segments_limits(key, ib or 0)
    rng = np.random.default_rng(3)
    specs = [(0, 0, 0), (wm, 0, 0), (1, 2, 1), (9, 10, 1)]
    waves = np.concatenate([[2], 2 + np.cumsum(rng.integers(0, wm + 1, size=41))]).astype(np.uint64)
    tb = Table(S.keys_for(int(waves[-1]) + 3 * (bm + 1), key, 9), waves)
    counts = S.plan(waves, 1, kb, bool(ib), UNBOUNDED)[1]
    assert counts[1:] == (0, 0, 0) and counts[0] > 30 and tb.n // (bm + 1) >= 3
    for largest, ob in ((False, 4), (True, 8)):
        _verify(gpu, tb, specs, largest, ib, _call(gpu, tb, specs, largest, ib, ob), "wave class only", _host_entry(gpu, tb, specs, largest, ib))
    blocks = np.cumsum([1, wm + 1, bm, 1025, bm - 1, wm + 9, bm]).astype(np.uint64)
    tb = Table(S.keys_for(int(blocks[-1]) + 2 * (bm + 1), key, 10), blocks)
    assert S.plan(blocks, 1, kb, bool(ib), UNBOUNDED)[1] == (0, 6, 0, 0) and tb.n // (bm + 1) >= 2
    for largest, ob in ((False, 8), (True, 4)):
        _verify(gpu, tb, specs, largest, ib, _call(gpu, tb, specs, largest, ib, ob), "block class only", _host_entry(gpu, tb, specs, largest, ib))


def test_counts_that_meet_the_grid_bounds(gpu):
    """every segment wave_max + 1 keys and len = n_segments * (wave_max + 1): the block class's count is its grid bound,
    len / (wave_max + 1); the same for the stream class with block_max + 1"""
    wm, bm, _sm, _mr = gpu.select_segments_limits("uint32", 4)
    specs = [(0, 0, 0), (wm, 0, 0), (bm, 0, 0), (1, 2, 2)]
    blocks = Table(S.keys_for(37 * (wm + 1), "uint32", 6), np.arange(38, dtype=np.uint64) * np.uint64(wm + 1))
    assert S.plan(blocks.off, 1, 4, True, UNBOUNDED)[1] == (0, 37, 0, 0) and blocks.n // (wm + 1) == 37
    _verify(gpu, blocks, specs, True, 4, _call(gpu, blocks, specs, True, 4, 8), "segments of wave_max + 1 keys")
    _verify(gpu, blocks, specs, False, None, _call(gpu, blocks, specs, False, None, 4), "segments of wave_max + 1 keys")
    streams = Table(S.keys_for(5 * (bm + 1), "uint32", 7), np.arange(6, dtype=np.uint64) * np.uint64(bm + 1))
    assert S.plan(streams.off, 1, 4, True, UNBOUNDED)[1] == (0, 0, 5, 0) and streams.n // (bm + 1) == 5
    _verify(gpu, streams, specs, False, 4, _call(gpu, streams, specs, False, 4, 4), "segments of block_max + 1 keys")
    _verify(gpu, streams, specs, True, 4, _call(gpu, streams, specs, True, 4, 8), "segments of block_max + 1 keys")


# ---- 5: rounds -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", (33, 70))
@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 4), ("uint64", 8)))
def test_more_specs_than_one_round(gpu, count, dtype, ib):
    wm, bm = gpu.select_segments_limits(dtype, ib or 0)[:2]
    off, n = S.residue_table([1, 3, wm, wm + 1, 1025, bm, bm + 1, 0, 2 * bm + 3, 40001], T.key_bytes(dtype))
    tb = Table(S.keys_for(n, dtype, 5), off)
    specs = Q.many_specs(count, count)
    for mode in (0, 1, 2):                                                  # the wrapper takes one mode per call: absolute ranks first
        chosen = [s for s in specs if s[1] == 0] + [(s[0], s[1], mode) for s in specs if s[1] != 0]
        largest = mode == 1
        _verify(gpu, tb, chosen, largest, ib, _call(gpu, tb, chosen, largest, ib, 4 if mode else 8), f"{count} specs",
                _host_entry(gpu, tb, chosen, largest, ib))


# ---- 6: what the device refuses -------------------------------------------------------------------------------------------------------

SMALL_SPECS = [(0, 0, 0), (1, 2, 0), (1, 1, 0)]


def _small_table(gpu, key="uint32", ib=None, extra=()):
    bm = gpu.select_segments_limits(key, ib or 0)[1]
    off = np.cumsum([2, 5, 700, 0, bm, 9] + list(extra)).astype(np.uint64)
    return Table(S.keys_for(int(off[-1]) + 4, key, 13), off), bm


def _invalid_tables(tb):
    """(name, offsets, len): a decreasing pair in the middle, a last offset past len"""
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
        bufs = _call(gpu, short, SMALL_SPECS, False, 4, ob, toff=toff)
        _table_error(gpu)
        _untouched(short, bufs, "async, " + name)
        # wait mode: the return code says so, nothing written, the error word clean
        raw_k, out_k, raw_i, out_i = _outputs(short, 3, 4)
        need = gpu.select_segments_device_offsets_scratch_bytes(short.n_seg, short.n, 3, "float32", 4)
        raw_s = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
        with pytest.raises(gpu.RdstHipError) as e:
            gpu.select_segments_device_offsets_tensor(short.t, toff, ranks=[0], quantiles=[(1, 2), (1, 1)], index=torch.int32,
                                                      scratch=raw_s[SLACK:SLACK + need], far_capacity=short.n, check=False, out=(out_k, out_i))
        assert e.value.code == ERR_ARG and ("non-decreasing" in str(e.value) or "past len" in str(e.value))
        gpu.device_status()
        _untouched(short, (raw_k, raw_i, raw_s, need), "wait, " + name)


def test_far_capacity_below_the_longest_far_segment(gpu, stream_max):
    import torch
    bm = gpu.select_segments_limits("uint64", 8)[1]
    tb = _small_table(gpu, "uint64", 8, extra=(2 * bm + 3,))[0]
    stream_max(bm)
    longest = tb.longest
    assert longest == 2 * bm + 3 and S.plan(tb.off, 1, 8, True, bm)[2] == longest
    raw_k, out_k, raw_i, out_i = _outputs(tb, 3, 8)
    need = gpu.select_segments_device_offsets_scratch_bytes(tb.n_seg, longest - 1, 3, "uint64", 8)
    raw_s = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu.RdstHipError) as e:
        gpu.select_segments_device_offsets_tensor(tb.t, tb.toff[8], ranks=[0], quantiles=[(1, 2), (1, 1)], index=torch.int64,
                                                  scratch=raw_s[SLACK:SLACK + need], far_capacity=longest - 1, check=False, out=(out_k, out_i))
    assert e.value.code == ERR_ARG and "far_capacity" in str(e.value)
    gpu.device_status()
    _untouched(tb, (raw_k, raw_i, raw_s, need), "far_capacity = longest - 1")
    _verify(gpu, tb, SMALL_SPECS, False, 8, _call(gpu, tb, SMALL_SPECS, False, 8, 4, far_capacity=longest), "far_capacity = longest",
            _host_entry(gpu, tb, SMALL_SPECS, False, 8))


# ---- 7: stream order, scratch reuse ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stream", ["default", "other"])
def test_offsets_from_a_cumsum_behind_a_kernel_that_writes_the_keys(gpu, stream):
    import torch
    wm, bm, _sm, _mr = gpu.select_segments_limits("uint32", 4)
    rng = np.random.default_rng(51)
    lengths = rng.integers(0, 41, size=2001)
    lengths[rng.choice(2001, size=8, replace=False)] = [wm, wm + 1, 600, bm, bm + 1, 2 * bm + 3, 0, 1]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    a = S.keys_for(int(off[-1]) + 5, "uint32", 23)
    tb = Table(np.zeros_like(a), off)
    src = H.to_device(a).view(torch.int32) ^ 0x5A5A5A5A
    tlen = torch.from_numpy(lengths).cuda()
    specs, specs32 = [(0, 0, 0), (20, 0, 0), (1, 2, 2), (9, 10, 2)], [(1, 2, 0)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if stream == "other" else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        for _ in range(4):                                                  # work in front of the write, so that the call is enqueued behind it
            src = (src ^ 0x1111) ^ 0x1111
        tb.t.view(torch.int32).copy_(src ^ 0x5A5A5A5A)
        toff = torch.zeros(len(lengths) + 1, dtype=torch.int64, device="cuda")
        toff[1:] = torch.cumsum(tlen, 0)                                    # queued on the stream; nothing comes to the host
        bufs = _call(gpu, tb, specs, True, 4, toff=toff)
        bufs32 = _call(gpu, tb, specs32, False, 4, toff=toff.to(torch.int32))
    torch.cuda.synchronize()
    tb.a = a                                                                # (what the producer wrote)
    _verify(gpu, tb, specs, True, 4, bufs, f"cumsum, {stream} stream")
    _verify(gpu, tb, specs32, False, 4, bufs32, f"cumsum, {stream} stream, int32")


def test_unsigned_offset_tensors(gpu):
    """uint32 and uint64 tables are taken as they are"""
    import torch
    tb, _bm = _small_table(gpu)
    for dt, ob in ((torch.uint32, 4), (torch.uint64, 8)):
        _verify(gpu, tb, SMALL_SPECS, False, None, _call(gpu, tb, SMALL_SPECS, False, None, toff=tb.toff[ob].view(dt)), str(dt))


def test_two_calls_back_to_back_on_one_scratch(gpu, stream_max):
    import torch
    bm = gpu.select_segments_limits("uint64", 0)[1]
    stream_max(2 * bm)
    off1 = np.cumsum([1, 3, 700, bm + 9, 3 * bm + 1]).astype(np.uint64)
    off2 = np.cumsum([5, 2 * bm + 3, 1, 513, bm + 1, 0, 7]).astype(np.uint64)
    t1, t2 = Table(S.keys_for(int(off1[-1]) + 1, "uint64", 1), off1), Table(S.keys_for(int(off2[-1]), "uint64", 2), off2)
    s1, s2 = [(0, 0, 0), (1, 2, 0), (1, 1, 0)], [(5, 0, 0), (1, 4, 1)]
    need = max(gpu.select_segments_device_offsets_scratch_bytes(t1.n_seg, t1.n, 3, "uint64"), gpu.select_segments_device_offsets_scratch_bytes(t2.n_seg, 0, 2, "uint64"))
    scratch = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    b1 = _call(gpu, t1, s1, False, None, 8, far_capacity=t1.n, scratch=scratch)    # a far segment, whose scratch lies behind the plan
    b2 = _call(gpu, t2, s2, True, None, 4, scratch=scratch)
    b3 = _call(gpu, t1, s2, True, None, 8, scratch=scratch)
    b4 = _call(gpu, t2, s1, False, None, 8, far_capacity=t2.n, scratch=scratch)
    _verify(gpu, t1, s1, False, None, b1, "first of four")
    _verify(gpu, t2, s2, True, None, b2, "second of four")
    _verify(gpu, t1, s2, True, None, b3, "third of four")
    _verify(gpu, t2, s1, False, None, b4, "fourth of four")
