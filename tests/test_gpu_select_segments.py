"""The segmented select (rdst_hip_select_segments_device) on the device.  Every case compares the WHOLE output
buffers — guard bands, rows, and the slots without a rank, all pre-filled — bit for bit with the numpy statement
(select_segments_inputs.expected_rows: per segment the element of a stable argsort by the mapped key at the rank the spec
stands for), and checks that the input is unchanged and that nothing was written before or behind the scratch the call was
told about."""
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


def _torch_index(ib):
    import torch
    return {None: None, 4: torch.int32, 8: torch.int64}[ib]


def _operands(specs):
    """the wrapper's two lists for a list of specs, in the same order: absolute ranks first (the tables here keep them so)"""
    ranks = [s[0] for s in specs if s[1] == 0]
    quantiles = [(s[0], s[1]) for s in specs if s[1] != 0]
    return ranks, quantiles


class Table:
    """keys on the device and a table of borders, with what does not depend on the specs computed once"""

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


def _call(gpu, tb, specs, largest, ib, scratch=None):
    """enqueues one call (check=False) on pre-filled, guarded outputs; returns what _verify needs.  The specs of one call share
    their mode (the wrapper's `method`); absolute ranks stand first."""
    import torch
    assert [s for s in specs if s[1] == 0] + [s for s in specs if s[1] != 0] == list(specs)
    modes = {s[2] for s in specs if s[1] != 0}
    assert len(modes) <= 1
    method = {0: "lower", 1: "higher", 2: "nearest"}[modes.pop() if modes else 0]
    per_key = 2 if T.is_wide(tb.key) else 1
    nr = len(specs)
    slots = tb.n_seg * nr
    raw_k = torch.full(((slots + 2 * GUARD) * per_key * tb.a.dtype.itemsize,), FILL_KEY, dtype=torch.uint8, device="cuda")
    out_k = raw_k.view(tb.t.dtype)[GUARD * per_key:(GUARD + slots) * per_key]
    raw_i = out_i = None
    if ib:
        raw_i = torch.full((slots + 2 * GUARD,), FILL_INDEX, dtype=_torch_index(ib), device="cuda")
        out_i = raw_i[GUARD:GUARD + slots]
    need = gpu.select_segments_scratch_bytes(tb.n_seg, tb.longest, nr, tb.name, ib or 0)
    if scratch is not None:                                                 # shared by several calls: the bands lie round the largest need
        assert scratch.numel() >= need + 2 * SLACK
        need = scratch.numel() - 2 * SLACK
    raw_s = scratch if scratch is not None else torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    ranks, quantiles = _operands(specs)
    got = gpu.select_segments_device_tensor(tb.t, tb.off, ranks=ranks, quantiles=quantiles, method=method, largest=largest, index=_torch_index(ib),
                                            scratch=raw_s[SLACK:SLACK + need], check=False, key=tb.key, out=(out_k, out_i))
    assert got[0] is out_k and got[1] is out_i
    return raw_k, raw_i, raw_s, need


def _verify(gpu, tb, specs, largest, ib, bufs, what=""):
    raw_k, raw_i, raw_s, need = bufs
    gpu.device_status()
    nr = len(specs)
    what = f"{what} {tb.name} segments = {tb.n_seg} specs = {specs[:6]} largest = {largest} index = {ib}"
    per_key = 2 if T.is_wide(tb.key) else 1
    want_k = np.full((tb.n_seg * nr + 2 * GUARD) * per_key * tb.a.dtype.itemsize, FILL_KEY, dtype=np.uint8).view(tb.a.dtype)
    rows_k = want_k[GUARD * per_key:(GUARD + tb.n_seg * nr) * per_key].reshape((tb.n_seg, nr, 2) if per_key == 2 else (tb.n_seg, nr))
    want_i = np.full(tb.n_seg * nr + 2 * GUARD, FILL_INDEX, dtype=np.int64)
    Q.expected_rows(tb.a, tb.off, specs, largest, tb.key, rows_k, want_i[GUARD:GUARD + tb.n_seg * nr].reshape(tb.n_seg, nr), tb.ordered(largest))
    got_k = raw_k.cpu().numpy()
    if not np.array_equal(got_k, want_k.view(np.uint8).reshape(-1)):
        bad = np.flatnonzero(got_k != want_k.view(np.uint8).reshape(-1))
        slot = int(bad[0]) // (per_key * tb.a.dtype.itemsize) - GUARD
        raise AssertionError(f"{what}: keys differ in {len(bad)} bytes, first in row {slot // nr} slot {slot % nr} "
                             f"(segment of {int(tb.off[slot // nr + 1] - tb.off[slot // nr]) if 0 <= slot < tb.n_seg * nr else '?'} keys)")
    if ib:
        got_i = raw_i.cpu().numpy().astype(np.int64)
        if not np.array_equal(got_i, want_i):
            slot = int(np.flatnonzero(got_i != want_i)[0]) - GUARD
            raise AssertionError(f"{what}: positions differ, first in row {slot // nr} slot {slot % nr}: {got_i[slot + GUARD]} != {want_i[slot + GUARD]}")
    assert np.array_equal(H.to_host(tb.t, tb.a.dtype).view(np.uint8), tb.a.view(np.uint8)), what + ": the input changed"
    assert bool((raw_s[:SLACK] == POISON).all()) and bool((raw_s[SLACK + need:] == POISON).all()), what + ": written outside the scratch"
    return want_k, want_i


def _check(gpu, tb, specs, largest=False, ib=None, what=""):
    return _verify(gpu, tb, specs, largest, ib, _call(gpu, tb, specs, largest, ib), what)


def _absolute(ranks):
    return [(int(r), 0, 0) for r in ranks]


@pytest.fixture
def stream_max(gpu):
    """the setter, put back to the default afterwards"""
    yield gpu.set_topk_segments_stream_max
    gpu.set_topk_segments_stream_max(0)


# ---- 1: every length at every start, every key type ---------------------------------------------------------------------------

def _length_table(gpu, key, ib):
    kb = T.key_bytes(key)
    wm, bm, _sm, mr = gpu.select_segments_limits(key, ib or 0)
    assert (wm, bm, mr) == (S.wave_max(kb), S.block_max(kb, bool(ib)), Q.MAX_RANKS)
    off, n = S.residue_table(S.segment_lengths(wm, bm), kb)
    return Table(S.keys_for(n, key, 11 + kb), off, key if T.is_wide(key) else None), wm


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_every_length_and_start_keys_only(gpu, key, kb):
    tb, wm = _length_table(gpu, key, None)
    for specs in Q.rank_sets(wm) + [[(1, 2, Q.HIGHER)]]:
        for largest in (False, True):
            _check(gpu, tb, specs, largest, None, "lengths")


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_every_length_and_start_with_an_index(gpu, key, ib):
    tb, wm = _length_table(gpu, key, ib)
    for specs in Q.rank_sets(wm)[:3] + [[(1, 2, Q.HIGHER)]]:
        for largest in (False, True):
            _check(gpu, tb, specs, largest, ib, "lengths")
    for largest in (False, True):
        _want_k, want_i = _check(gpu, tb, Q.rank_sets(wm)[3], largest, ib, "lengths")
    lens = tb.off[1:] - tb.off[:-1]
    short = np.flatnonzero(lens <= wm)                                      # the absolute rank wave_max: those rows keep the fill
    rows = want_i[GUARD:-GUARD].reshape(tb.n_seg, -1)
    assert len(short) and bool((rows[short, 0] == FILL_INDEX).all()) and bool((rows[np.flatnonzero(lens > wm), 0] != FILL_INDEX).all())


# ---- 2: the stream class --------------------------------------------------------------------------------------------------------

DEPTH_DTYPES = ("uint16", "int32", "float32", "uint64", "float64")


@pytest.mark.parametrize("dtype", DEPTH_DTYPES)
def test_stream_class_at_every_depth(gpu, dtype):
    """(a) segments of 2 bm + 3 keys whose mapped keys share their top 0, 12, 24 ... bits, up to all of them: the select takes
    1, 2, 3 ... levels (tests/test_select_segments_inputs.py holds the depth of every segment), starts of three residues"""
    kb = np.dtype(dtype).itemsize
    for ib in ((None, 4) if kb == 4 else (None, 8) if kb == 8 else (None,)):
        bm = gpu.select_segments_limits(dtype, ib or 0)[1]
        n = 2 * bm + 3
        parts = [S.shared_digits(n, dtype, j, 40 + j) for j in range(T.key_levels(kb) + 1)]
        off = np.cumsum([1] + [n] * len(parts)).astype(np.uint64)
        tb = Table(np.concatenate([parts[0][:1]] + parts + [parts[0][:2]]), off)
        for specs in ([(1, 2, 0)], _absolute([0, n - 1]) + [(1, 4, 1), (3, 4, 1)]):
            for largest in (False, True):
                _check(gpu, tb, specs, largest, ib, "depth")


@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 8), ("int64", 4), ("uint16", None)))
def test_exactly_a_tile_on_the_final_prefix_and_one_more(gpu, dtype, ib):
    """(b) m == TILE after the first level: the select stops; TILE + 1: it takes a second level.  More keys lie before the prefix
    than the stage could hold: they are only counted"""
    bm = gpu.select_segments_limits(dtype, ib or 0)[1]
    n = 2 * bm + 3
    for extra in (0, 1):
        a, r = Q.prefix_border(dtype, bm, n, extra, 5 + extra)
        levels, c_below, m = Q.stream_select(a, r, False, bm)
        assert levels == 1 + extra and c_below + m > bm
        tb = Table(np.concatenate([a[:3], a]), np.array([3, 3 + n], dtype=np.uint64))
        for ranks in ([r], [c_below, r, c_below + m - 1]):
            for largest in (False, True):
                _check(gpu, tb, _absolute(ranks if not largest else [n - 1 - x for x in ranks]), largest, ib, f"TILE + {extra} on the prefix")


@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("uint32", 4), ("float64", 8), ("uint8", None), ("u128", None)))
def test_ranks_that_share_a_stage_and_ranks_that_do_not(gpu, dtype, ib):
    """(c) neighbours on one prefix are answered from one stage; 0 and n_s - 1 lie on disjoint prefixes and descend apart"""
    key = dtype if T.is_wide(dtype) else None
    bm = gpu.select_segments_limits(dtype, ib or 0)[1]
    n = 2 * bm + 3
    a = T.random_keys(n, dtype, 77)
    _lv, c_below, m = Q.stream_select(a, n // 2, False, bm, key)
    shared = sorted({c_below, min(c_below + 1, c_below + m - 1), c_below + m - 1})
    assert Q.descents(a, shared, False, bm, key) == 1 and Q.descents(a, [0, n - 1], False, bm, key) == 2
    tb = Table(np.concatenate([a[:1], a]), np.array([1, 1 + n], dtype=np.uint64), key)
    for ranks in (shared, [0, n - 1], [n - 1, 0, c_below, n // 2, n - 1, 0] + shared):
        for largest in (False, True):
            _check(gpu, tb, _absolute(ranks), largest, ib, "stages")


@pytest.mark.parametrize("dtype,ib", (("uint32", 4), ("float64", 8), ("int64", 4), ("uint32", None), ("uint16", None)))
def test_all_equal_segment_windows(gpu, dtype, ib):
    """(d) 3 TILE + 5 equal keys: the digits are exhausted with m > TILE; with an index the position of rank r is r itself, read
    from the window of TILE ordinals that holds it (ranks in the windows 0, 1, 2 and 3; two share a window)"""
    bm = gpu.select_segments_limits(dtype, ib or 0)[1]
    n = 3 * bm + 5
    one = T.random_keys(1, dtype, 9)
    tb = Table(np.concatenate([one, np.repeat(one, n)]), np.array([1, 1 + n], dtype=np.uint64))
    ranks = Q.window_ranks(bm)
    for largest in (False, True):
        bufs = _call(gpu, tb, _absolute(ranks), largest, ib)
        _verify(gpu, tb, _absolute(ranks), largest, ib, bufs, "windows")
        if ib:
            assert bufs[1].cpu().numpy()[GUARD:GUARD + len(ranks)].tolist() == ranks        # position equals rank
    # equal keys beside others: a prefix of more than TILE equal keys inside a segment
    other = T.random_keys(bm, dtype, 10)
    a = np.concatenate([other, np.repeat(one, n), other])
    tb = Table(a, np.array([0, len(a)], dtype=np.uint64))
    below = int((H.mapped_key(other) < H.mapped_key(one)[0]).sum()) * 2
    for largest in (False, True):
        _check(gpu, tb, _absolute([0, below + 3, below + bm + 1, below + 3 * bm + 4, len(a) - 1]), largest, ib, "windows inside")


@pytest.mark.parametrize("dtype,ib", (("float32", None), ("float32", 4), ("float64", None), ("float64", 8)))
def test_zeros_and_nans_on_the_rank(gpu, dtype, ib):
    """(e) -0.0 and +0.0 are distinct keys, and so are NaNs of different payloads: the first and last rank of every run"""
    bm = gpu.select_segments_limits(dtype, ib or 0)[1]
    n = 2 * bm + 3
    a, ranks = Q.float_zero_nan_segment(dtype, n, 9)
    tb = Table(np.concatenate([a[:2], a, a[:700]]), np.array([2, 2 + n, 2 + n + 700], dtype=np.uint64))
    for largest in (False, True):
        _check(gpu, tb, _absolute(ranks if not largest else [n - 1 - r for r in ranks]), largest, ib, "zeros and NaNs")
        _check(gpu, tb, [(1, 2, 0), (1, 3, 0), (2, 3, 0)], largest, ib, "zeros and NaNs")


# ---- 3: rounds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", (33, 65))
@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 4), ("uint64", 8)))
def test_more_specs_than_one_round(gpu, count, dtype, ib):
    wm, bm = gpu.select_segments_limits(dtype, ib or 0)[:2]
    off, n = S.residue_table([1, 3, wm, wm + 1, 1025, bm, bm + 1, 0, 2 * bm + 3, 40001], T.key_bytes(dtype))
    tb = Table(S.keys_for(n, dtype, 5), off)
    specs = Q.many_specs(count, count)
    for mode in (0, 1, 2):                                                  # the wrapper takes one mode per call: absolute ranks first
        chosen = [s for s in specs if s[1] == 0] + [(s[0], s[1], mode) for s in specs if s[1] != 0]
        _check(gpu, tb, chosen, mode == 1, ib, f"{count} specs")


# ---- 4: the far class ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 4), ("int64", 8), ("uint16", None)))
def test_stream_and_far_class_give_the_same_bits(gpu, stream_max, dtype, ib):
    bm = gpu.select_segments_limits(dtype, ib or 0)[1]
    off = np.cumsum([1, bm + 1, 2 * bm + 3, 0, bm + 1025, 5]).astype(np.uint64)
    tb = Table(S.keys_for(int(off[-1]) + 2, dtype, 17), off)
    specs = _absolute([0, bm + 1024, bm + 1025]) + [(1, 2, 2), (1, 10, 2), (1, 1, 2), (1, 2, 2)]
    for largest in (False, True):
        outs = []
        for border in (0, bm):
            stream_max(border)
            assert gpu.topk_segments_plan(off, len(tb.a), 1, dtype, ib or 0)[1] == ((1, 0, 0, 3) if border else (1, 0, 3, 0))
            bufs = _call(gpu, tb, specs, largest, ib)
            _verify(gpu, tb, specs, largest, ib, bufs, f"stream_max = {border}")
            outs.append(bufs)
        assert bool((outs[0][0] == outs[1][0]).all()) and (not ib or bool((outs[0][1] == outs[1][1]).all()))


# ---- 5: streams and shapes -------------------------------------------------------------------------------------------------------

def test_two_calls_on_a_side_stream_share_one_scratch(gpu, stream_max):
    import torch
    bm = gpu.select_segments_limits("uint64", 0)[1]
    off1, n1 = S.residue_table([3, 700, bm + 9, 3 * bm + 1], 8)
    off2, n2 = S.residue_table([2 * bm + 3, 1, 513, bm + 1], 8)
    stream_max(2 * bm + 3)                                                   # (3 bm + 1 keys: the far class, whose scratch lies behind the table)
    side = torch.cuda.Stream()
    t1, t2 = Table(S.keys_for(n1, "uint64", 1), off1), Table(S.keys_for(n2, "uint64", 2), off2)
    s1, s2 = [(0, 0, 0), (1, 2, 0), (1, 1, 0)], [(5, 0, 0), (1, 4, 1)]
    need = max(gpu.select_segments_scratch_bytes(t1.n_seg, t1.longest, 3, "uint64"), gpu.select_segments_scratch_bytes(t2.n_seg, t2.longest, 2, "uint64"))
    assert need > gpu.select_segments_scratch_bytes(t2.n_seg, t2.longest, 2, "uint64")
    scratch = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b1 = _call(gpu, t1, s1, False, None, scratch)
        b2 = _call(gpu, t2, s2, True, None, scratch)
        b3 = _call(gpu, t1, s2, True, None, scratch)
    side.synchronize()
    _verify(gpu, t1, s1, False, None, b1, "first of three")
    _verify(gpu, t2, s2, True, None, b2, "second of three")
    _verify(gpu, t1, s2, True, None, b3, "third of three")


@pytest.mark.parametrize("n", (1, 700, 40000))
def test_one_segment(gpu, n):
    tb = Table(S.keys_for(n + 4, "int32", 3), np.array([2, 2 + n], dtype=np.uint64))
    _check(gpu, tb, [(0, 0, 0), (n - 1, 0, 0), (n, 0, 0), (1, 2, 1)], False, 8, "one segment")


@pytest.mark.parametrize("dtype", ("uint32", "float32"))
def test_rows_of_a_matrix_against_numpy_sort(gpu, dtype):
    import torch
    rows, cols = 37, 1000
    rng = np.random.default_rng(12)
    a = (rng.integers(0, 5000, size=rows * cols).astype(dtype) if dtype == "uint32" else rng.standard_normal(rows * cols).astype(dtype)).reshape(rows, cols)
    t = H.to_device(a.reshape(-1)).reshape(rows, cols)
    keys, index = gpu.select_rows_tensor(t, ranks=[0, cols - 1], quantiles=[0.5, 0.1, 0.9], index=torch.int64)
    srt = np.sort(a, axis=1)
    got = H.to_host(keys.reshape(-1), dtype).reshape(rows, 5)
    assert keys.shape == (rows, 5) and index.shape == (rows, 5)
    assert np.array_equal(got, srt[:, [0, cols - 1, (cols - 1) // 2, (cols - 1) // 10, 9 * (cols - 1) // 10]])
    assert np.array_equal(np.take_along_axis(a, index.cpu().numpy(), axis=1), got)
    largest, none = gpu.select_rows_tensor(t, quantiles=[0, (1, 2)], method="higher", largest=True)
    assert none is None and np.array_equal(H.to_host(largest.reshape(-1), dtype).reshape(rows, 2), srt[:, [cols - 1, cols - 1 - cols // 2]])
