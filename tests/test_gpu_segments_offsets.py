"""The segmented sort with its table of borders in device memory (rdst_hip_sort_segments_device_offsets / _pairs_;
rdst_amd.sort_segments_device_offsets_tensor): the device plan must produce rdst_segments_plan's work list item for item,
every segment must end exactly as the host-offsets entry leaves it in both modes (tmp=None: fully asynchronous; with tmp:
long segments too), an invalid table must change nothing and be reported, and nothing outside the segments, the scratch
and the tmps may be written.  Every length comes from segments_limits."""
import ctypes
import re

import numpy as np
import pytest

from helpers import PAIR_WIDTHS, Bands, expected_pairs, key_dtype, position_values, same_bits, to_device, to_host
from segments_offsets_inputs import HEAD_GAP, KEY_OF_WIDTH, LIMIT_PAIRS, TAIL_GAP, class_counts, many_lengths, offsets_of
from test_gpu_segments import KEYS, _np_dtype, _random, check_segments, edges_offsets, fill_segments

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_DEVICE = -1, -5
TABLE_BIT = 16          # ERR_SEGMENTS_TABLE of rdst_segments.hip


def _torch_offsets(off, ob):
    import torch
    return torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dtype=torch.int32 if ob == 4 else torch.int64).cuda()


def _wide(key):
    return "u128" if key == "u128" else None


def _table_error(gpu):
    """device_status() must raise RDST_ERR_DEVICE with the table bit in the word; returns the word"""
    with pytest.raises(gpu.RdstHipError) as e:
        gpu.device_status()
    assert e.value.code == ERR_DEVICE
    word = int(re.search(r"device error word = 0x([0-9a-f]+)", str(e.value)).group(1), 16)
    assert word & TABLE_BIT, hex(word)
    assert "16 = segmented sort" in str(e.value)
    return word


# ---- 1. the plan ------------------------------------------------------------------------------------------------------------

def _plan_tables(wave_max, block_max):
    """(name, offsets, n) of the plan parity cases"""
    yield ("EDGES",) + edges_offsets(wave_max, block_max)
    for name, length in (("one wave-class segment", wave_max), ("one block-class segment", wave_max + 1), ("one long segment", block_max + 1),
                         ("one empty segment", 0), ("one one-key segment", 1)):
        yield (name,) + offsets_of([length])
    yield ("two segments", ) + offsets_of([block_max, 2])
    yield ("only empty segments",) + offsets_of([0] * 50)
    lengths = many_lengths(wave_max, block_max)
    yield ("70 001 segments",) + offsets_of(lengths)
    # 100 000 empty segments over 1 000 keys: every bound the host can state lies far above the counts (all zero)
    yield "100 000 empty segments", np.full(100_001, 500, dtype=np.int64), 1000


@pytest.mark.parametrize("ob", [4, 8])
@pytest.mark.parametrize("kb,vb", LIMIT_PAIRS)
def test_device_plan_equals_the_host_plan(gpu, kb, vb, ob):
    key = KEY_OF_WIDTH[kb]
    wave_max, block_max = gpu.segments_limits(key, vb)
    for name, off, n in _plan_tables(wave_max, block_max):
        want = gpu.segments_plan(off, n, key, vb)
        got = gpu.segments_plan_device(_torch_offsets(off, ob), n, key, vb)
        what = f"({kb}, {vb}) {ob}-byte offsets, {name}"
        assert got[3] == 0, what
        assert got[1] == want[1] and got[2] == want[2], f"{what}: counts {got[1]} / {want[1]}, tmp_elems {got[2]} / {want[2]}"
        if got[0] != want[0]:
            first = next(i for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b)
            raise AssertionError(f"{what}: item {first} is {got[0][first]}, the host plan has {want[0][first]}")
        if name == "70 001 segments":
            assert want[1] == class_counts(many_lengths(wave_max, block_max), wave_max, block_max)[0]
    gpu.device_status()      # the hook leaves the error word alone


def test_plan_hook_reports_invalid_tables_as_flags(gpu):
    off, n = edges_offsets(*gpu.segments_limits("uint32"))
    bad = off.copy()
    bad[7], bad[8] = off[8], off[7]
    assert bad[8] < bad[7]
    for ob in (4, 8):
        assert gpu.segments_plan_device(_torch_offsets(bad, ob), n, "uint32")[3] == 1
        assert gpu.segments_plan_device(_torch_offsets(off, ob), int(off[-1]) - 1, "uint32")[3] == 2
        assert gpu.segments_plan_device(_torch_offsets(bad, ob), int(off[-1]) - 1, "uint32")[3] == 3
        neg = off.copy()
        neg[3] = -1          # read as unsigned: far past everything, so the next border lies below it
        assert gpu.segments_plan_device(_torch_offsets(neg, ob), n, "uint32")[3] & 1
    gpu.device_status()


# ---- 2., 3. keys ----------------------------------------------------------------------------------------------------------------

def _edges_case(gpu, key, val_bytes=0, seed=3, with_long=True, few=None):
    wave_max, block_max = gpu.segments_limits(key, val_bytes)
    off, n = edges_offsets(wave_max, block_max, with_long=with_long)
    return fill_segments(_random(n, key, seed), off, key, few=few), off, n, block_max


@pytest.mark.parametrize("ob", [4, 8])
@pytest.mark.parametrize("key", KEYS)
def test_asynchronous_mode_equals_the_host_offsets_entry(gpu, key, ob):
    a, off, n, _block_max = _edges_case(gpu, key, with_long=False)
    _items, counts, tmp_elems = gpu.segments_plan(off, n, key)
    assert counts == (7, 6, 0) and tmp_elems == 0       # 7 waves: the last workgroup of the wave class has an idle wave
    t, t2 = to_device(a), to_device(a)
    gpu.sort_segments_device_offsets_tensor(t, _torch_offsets(off, ob), check=False, key=_wide(key))
    gpu.device_status()
    got = to_host(t, _np_dtype(key))
    check_segments(got, a, off, key, f"{key}, {ob}-byte offsets")
    gpu.sort_segments_device_tensor(t2, off, key=_wide(key))
    assert same_bits(to_host(t2, _np_dtype(key)), got)


@pytest.mark.parametrize("key,ob", [("uint8", 4), ("int16", 8), ("float32", 4), ("int64", 8), ("u128", 4), ("uint32", 8)])
def test_tmp_mode_sorts_long_segments_too(gpu, key, ob):
    import torch
    a, off, n, block_max = _edges_case(gpu, key, seed=13)
    longest = 2 * block_max + 17
    assert gpu.segments_plan(off, n, key)[1:] == ((7, 6, 2), longest)
    per_key = 2 if key == "u128" else 1
    t, t2 = to_device(a), to_device(a)
    toff = _torch_offsets(off, ob)
    tmp = torch.empty((longest * per_key,), dtype=t.dtype, device=t.device)       # exactly the longest
    gpu.sort_segments_device_offsets_tensor(t, toff, tmp=tmp, check=False, key=_wide(key))
    gpu.device_status()
    got = to_host(t, _np_dtype(key))
    check_segments(got, a, off, key, f"{key} tmp mode")
    gpu.sort_segments_device_tensor(t2, off, key=_wide(key))
    assert same_bits(to_host(t2, _np_dtype(key)), got)
    # one element less: refused by the return code, nothing sorted, nothing left in the error word
    t3 = to_device(a)
    with pytest.raises(gpu.RdstHipError) as e:
        gpu.sort_segments_device_offsets_tensor(t3, toff, tmp=tmp[:(longest - 1) * per_key], check=False, key=_wide(key))
    assert e.value.code == ERR_ARG and "tmp_elems" in str(e.value)
    gpu.device_status()
    assert same_bits(to_host(t3, _np_dtype(key)), a)
    # a larger tmp, and a table without long segments in this mode
    t4 = to_device(a)
    short, _n = edges_offsets(*gpu.segments_limits(key), with_long=False)
    big = torch.empty(((longest + 100) * per_key,), dtype=t.dtype, device=t.device)
    gpu.sort_segments_device_offsets_tensor(t4, _torch_offsets(short, ob), tmp=big, key=_wide(key))
    check_segments(to_host(t4, _np_dtype(key)), a, short, key, f"{key} tmp mode, no long segment")


# ---- 4. pairs -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["asynchronous", "tmp"])
@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_pairs_equal_the_host_offsets_entry_and_are_stable(gpu, kb, vb, mode):
    import torch
    key = key_dtype(kb, {(4, 4): "u", (4, 8): "i", (8, 4): "f", (8, 8): "u"}[(kb, vb)])
    vdtype = f"uint{8 * vb}"
    keys, off, n, block_max = _edges_case(gpu, key, vb, seed=5, with_long=mode == "tmp", few=3)   # three distinct keys per segment at most
    vals = position_values(n, vdtype)
    tk, tv, hk, hv = to_device(keys), to_device(vals), to_device(keys), to_device(vals)
    toff = _torch_offsets(off, 4 if vb == 4 else 8)
    tmp = tmp_values = None
    if mode == "tmp":
        longest = 2 * block_max + 17
        tmp, tmp_values = torch.empty((longest,), dtype=tk.dtype, device=tk.device), torch.empty((longest,), dtype=tv.dtype, device=tv.device)
    gpu.sort_segments_device_offsets_tensor(tk, toff, tmp=tmp, values=tv, tmp_values=tmp_values, check=False)
    gpu.device_status()
    gk, gv = to_host(tk, key), to_host(tv, vdtype)
    gpu.sort_segments_device_tensor(hk, off, values=hv)
    assert same_bits(gk, to_host(hk, key)) and same_bits(gv, to_host(hv, vdtype))
    lo0, hi0 = int(off[0]), int(off[-1])
    assert same_bits(gk[:lo0], keys[:lo0]) and same_bits(gk[hi0:], keys[hi0:])
    assert same_bits(gv[:lo0], vals[:lo0]) and same_bits(gv[hi0:], vals[hi0:])
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        ek, ev = expected_pairs(keys[lo:hi], vals[lo:hi])
        assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), f"({kb}, {vb}) {mode}: segment {s} of length {hi - lo}"


# ---- 5. offsets that never visit the host -----------------------------------------------------------------------------------------

def _ragged_lengths(gpu, key, seed):
    wave_max, block_max = gpu.segments_limits(key)
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 41, size=3001)
    lengths[rng.choice(3001, size=12, replace=False)] = [wave_max, wave_max + 1, 600, block_max, 1023, 1025, 3, 64, 65, 2000, block_max - 1, 0]
    return lengths


@pytest.mark.parametrize("stream", ["default", "other"])
def test_offsets_from_a_cumsum_on_the_device(gpu, stream):
    import torch
    key = "uint32"
    lengths = _ragged_lengths(gpu, key, 51)
    n = int(lengths.sum()) + TAIL_GAP
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    a = _random(n, key, 52)
    b = _random(n, key, 53)
    t, t2 = to_device(a), to_device(b)
    tlen = torch.from_numpy(lengths).cuda()
    scratch = torch.empty(gpu.segments_device_offsets_scratch_bytes(len(lengths)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if stream == "other" else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        toff = torch.zeros(len(lengths) + 1, dtype=torch.int64, device="cuda")
        toff[1:] = torch.cumsum(tlen, 0)                                       # queued on the stream; nothing comes to the host
        gpu.sort_segments_device_offsets_tensor(t, toff, scratch=scratch, check=False)
        # a second call right behind it with the same scratch, its table the int32 image of the first
        toff32 = toff.to(torch.int32)
        gpu.sort_segments_device_offsets_tensor(t2, toff32, scratch=scratch, check=False)
        gpu.device_status()
    torch.cuda.synchronize()
    check_segments(to_host(t, key), a, off, key, f"cumsum, {stream} stream")
    check_segments(to_host(t2, key), b, off, key, f"cumsum, {stream} stream, second call")


# ---- 6. invalid tables --------------------------------------------------------------------------------------------------------------

def _invalid_tables(off, n, block_max):
    """(name, offsets, len) of the three tables the asynchronous mode must refuse"""
    dec = off.copy()
    mid = len(off) // 2
    dec[mid] = off[mid + 1] + 1
    assert dec[mid + 1] < dec[mid]
    yield "a decreasing pair in the middle", dec, n
    yield "a last offset of len + 1", off, int(off[-1]) - 1
    long_off, long_n = offsets_of([5, block_max + 1, 9])
    yield "a segment of block_max + 1 without tmp", long_off, long_n


@pytest.mark.parametrize("ob", [4, 8])
@pytest.mark.parametrize("pairs", [False, True])
def test_invalid_tables_change_nothing_and_are_reported(gpu, ob, pairs):
    import torch
    key, vb = ("uint64", 4) if pairs else ("float32", 0)
    a, off, n, block_max = _edges_case(gpu, key, vb, seed=61, with_long=False)
    vals = position_values(n, "uint32")
    gpu.device_status()
    for name, bad, bad_n in _invalid_tables(off, n, block_max):
        size = max(n, bad_n + 1)
        k0 = _random(size, key, 62)
        v0 = position_values(size, "uint32")
        tk, tv = to_device(k0), to_device(v0)
        gpu.sort_segments_device_offsets_tensor(tk[:bad_n], _torch_offsets(bad, ob), values=tv[:bad_n] if pairs else None, check=False)
        _table_error(gpu)
        gpu.device_status()                                   # reported once
        assert same_bits(to_host(tk, key), k0), name
        assert same_bits(to_host(tv, "uint32"), v0), name
        # a valid call afterwards sorts
        tk, tv = to_device(a), to_device(vals)
        gpu.sort_segments_device_offsets_tensor(tk, _torch_offsets(off, ob), values=tv if pairs else None)
        check_segments(to_host(tk, key), a, off, key, f"after {name}")
        # tmp mode: the host sees the flags
        if "tmp" not in name:
            tk, tv = to_device(k0), to_device(v0)
            tmp, tmpv = torch.empty(64, dtype=tk.dtype, device="cuda"), torch.empty(64, dtype=tv.dtype, device="cuda")
            with pytest.raises(gpu.RdstHipError) as e:
                gpu.sort_segments_device_offsets_tensor(tk[:bad_n], _torch_offsets(bad, ob), tmp=tmp, values=tv[:bad_n] if pairs else None,
                                                        tmp_values=tmpv if pairs else None, check=False)
            assert e.value.code == ERR_ARG and ("non-decreasing" in str(e.value) or "past len" in str(e.value)), name
            gpu.device_status()                               # a clean error word
            assert same_bits(to_host(tk, key), k0) and same_bits(to_host(tv, "uint32"), v0), name


# ---- 7. bounds ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["asynchronous", "tmp"])
@pytest.mark.parametrize("ob", [4, 8])
def test_nothing_outside_the_buffers_is_written(gpu, ob, mode):
    from rdst_amd import _lib
    from rdst_amd.radix_sort import key_info
    import torch
    key, vdtype = "int32", "uint64"
    kind, nbytes, levels = key_info(key)
    wave_max, block_max = gpu.segments_limits(key, 8)
    off, n = edges_offsets(wave_max, block_max, with_long=mode == "tmp")
    keys = fill_segments(_random(n, key, 71), off, key)
    vals = position_values(n, vdtype)
    longest = 2 * block_max + 17 if mode == "tmp" else 0
    table = np.ascontiguousarray(off, dtype=np.int32 if ob == 4 else np.int64)
    need = gpu.segments_device_offsets_scratch_bytes(len(off) - 1)
    bands = {"keys": Bands([("keys", keys, 4)], seed=1), "vals": Bands([("vals", vals, 8)], seed=2),
             "offsets": Bands([("offsets", table, 4 if ob == 4 else 8)], seed=3),            # 4-byte offsets: aligned to 4 bytes only
             "scratch": Bands([("scratch", ((need,), "uint8"), 0)], seed=4),
             "tmp": Bands([("tmp", ((max(longest, 1),), keys.dtype), 12)], seed=5), "tmpv": Bands([("tmpv", ((max(longest, 1),), vals.dtype), 8)], seed=6)}
    assert bands["offsets"]["offsets"].data_ptr() % 8 == (4 if ob == 4 else 0) and bands["scratch"]["scratch"].data_ptr() % 256 == 0
    vp = ctypes.c_void_p
    ptr = lambda name: vp(bands[name][name].data_ptr())   # noqa: E731
    s = vp(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    what = f"{ob}-byte offsets, {mode} mode"
    _lib.check(lib.rdst_hip_sort_segments_pairs_device_offsets(ptr("keys"), ptr("vals"), ptr("tmp") if longest else None, ptr("tmpv") if longest else None,
                                                               longest, n, ptr("offsets"), ob, len(off) - 1, nbytes, kind, levels, 8, ptr("scratch"),
                                                               need, s))
    gpu.device_status()
    gk, gv = to_host(bands["keys"]["keys"], key), to_host(bands["vals"]["vals"], vdtype)
    for sgm in range(len(off) - 1):
        lo, hi = int(off[sgm]), int(off[sgm + 1])
        ek, ev = expected_pairs(keys[lo:hi], vals[lo:hi])
        assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), f"{what}: segment {sgm}"
    lo0, hi0 = int(off[0]), int(off[-1])
    assert same_bits(gk[:lo0], keys[:lo0]) and same_bits(gk[hi0:], keys[hi0:]) and same_bits(gv[:lo0], vals[:lo0]) and same_bits(gv[hi0:], vals[hi0:])
    for name, b in bands.items():
        b.check(f"{what}: {name}", untouched=("offsets",) if name == "offsets" else (("tmp",) if name == "tmp" and not longest else ()))
    # keys only, through the same buffers
    kb2 = Bands([("keys", keys, 4)], seed=7)
    _lib.check(lib.rdst_hip_sort_segments_device_offsets(vp(kb2["keys"].data_ptr()), ptr("tmp") if longest else None, longest, n, ptr("offsets"), ob,
                                                         len(off) - 1, nbytes, kind, levels, ptr("scratch"), need, s))
    gpu.device_status()
    check_segments(to_host(kb2["keys"], key), keys, off, key, what + " (keys only)")
    kb2.check(what + " (keys only)")
    for name in ("offsets", "scratch", "tmp"):
        bands[name].check(f"{what} (keys only): {name}", untouched=("offsets",) if name == "offsets" else ())
