"""The segmented sort that never visits the host (rdst_hip_sort_segments_device_offsets_nowait / _pairs_;
rdst_amd.sort_segments_device_offsets_nowait_tensor): segments beyond block_max take the tiled device route.  Every segment
must end bit for bit as numpy sorts it (np.sort per segment; the stable order for pairs) AND as the host-offsets entry
sort_segments_device_tensor leaves it; an invalid table must change nothing and be reported once; nothing outside the
segments, the long segments' positions in tmp, and the scratch may be written.  Every length comes from segments_limits."""
import ctypes
import re

import numpy as np
import pytest

from helpers import PAIR_WIDTHS, Bands, expected_pairs, key_dtype, position_values, same_bits, to_device, to_host
from segments_nowait_inputs import (DIGIT_SHAPES, MANY_LONG, border_lengths, degenerate_tables, digit_shape_keys, four_value_keys,
                                    invalid_tables, long_count, many_items_lengths, plant_float32_specials, tile_count)
from segments_offsets_inputs import HEAD_GAP, TAIL_GAP, offsets_of
from test_gpu_segments import _np_dtype, _random, check_segments

pytestmark = pytest.mark.gpu

ERR_DEVICE = -5
TABLE_BIT = 16          # ERR_SEGMENTS_TABLE of rdst_segments.hip


def _torch_offsets(off, ob):
    import torch
    return torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dtype=torch.int32 if ob == 4 else torch.int64).cuda()


def _wide(key):
    return "u128" if key == "u128" else None


def _table_error(gpu):
    """device_status() must raise RDST_ERR_DEVICE with the table bit in the word"""
    with pytest.raises(gpu.RdstHipError) as e:
        gpu.device_status()
    assert e.value.code == ERR_DEVICE
    word = int(re.search(r"device error word = 0x([0-9a-f]+)", str(e.value)).group(1), 16)
    assert word & TABLE_BIT, hex(word)


def _sort_both_ways(gpu, a, off, key, ob, what):
    """the nowait entry and the host-offsets entry on copies of `a`; checks both against numpy and each other; returns the tmp"""
    import torch
    t, t2 = to_device(a), to_device(a)
    tmp0 = _random(len(a), key, 977)
    tmp = to_device(tmp0)
    gpu.sort_segments_device_offsets_nowait_tensor(t, _torch_offsets(off, ob), tmp=tmp, check=False, key=_wide(key))
    gpu.device_status()
    got = to_host(t, _np_dtype(key))
    check_segments(got, a, off, key, what)
    gpu.sort_segments_device_tensor(t2, off, key=_wide(key))
    assert same_bits(to_host(t2, _np_dtype(key)), got), what
    return tmp0, to_host(tmp, _np_dtype(key))


def _check_tmp(tmp0, tmp1, off, block_max, what):
    """tmp changed at most inside the long segments"""
    keep = np.ones(len(tmp0), dtype=bool)
    for s in range(len(off) - 1):
        if off[s + 1] - off[s] > block_max:
            keep[int(off[s]):int(off[s + 1])] = False
    assert same_bits(tmp0[keep], tmp1[keep]), f"{what}: tmp changed outside the long segments"


# ---- 1. tile borders ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ob", [4, 8])
@pytest.mark.parametrize("key", ["uint8", "int16", "uint32", "float32", "int64", "u128"])
def test_tile_borders(gpu, key, ob):
    wave_max, block_max = gpu.segments_limits(key)
    lengths = border_lengths(wave_max, block_max)
    assert long_count(lengths, block_max) == 6 and tile_count(lengths, block_max) == 18
    off, n = offsets_of(lengths)
    assert off[0] == HEAD_GAP and n - off[-1] == TAIL_GAP
    a = _random(n, key, 3)
    if key == "float32":
        plant_float32_specials(a, off)
    what = f"{key}, {ob}-byte offsets"
    tmp0, tmp1 = _sort_both_ways(gpu, a, off, key, ob, what)
    _check_tmp(tmp0, tmp1, off, block_max, what)


# ---- 2. digit shapes inside a long segment -------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["uint32", "uint64"])
def test_digit_shapes_inside_a_long_segment(gpu, key):
    wave_max, T = gpu.segments_limits(key)
    n_long = 3 * T + 5
    off, n = offsets_of([9, n_long, 40])
    for shape in DIGIT_SHAPES:
        a = _random(n, key, 5)
        a[off[1]:off[2]] = digit_shape_keys(shape, n_long, key, T)
        _sort_both_ways(gpu, a, off, key, 8, f"{key}, {shape}")


# ---- 3. pairs --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_pairs_are_stable_across_tiles(gpu, kb, vb):
    key = key_dtype(kb, {(4, 4): "u", (4, 8): "i", (8, 4): "f", (8, 8): "u"}[(kb, vb)])
    vdtype = f"uint{8 * vb}"
    wave_max, T = gpu.segments_limits(key, vb)
    lengths = [T + 1, 3, 2 * T, wave_max + 9, 4 * T + 3]
    off, n = offsets_of(lengths)
    keys = four_value_keys(n, key, 7)
    vals = position_values(n, vdtype)
    tk, tv, hk, hv = to_device(keys), to_device(vals), to_device(keys), to_device(vals)
    gpu.sort_segments_device_offsets_nowait_tensor(tk, _torch_offsets(off, 4 if vb == 4 else 8), values=tv, check=False)
    gpu.device_status()
    gk, gv = to_host(tk, key), to_host(tv, vdtype)
    lo0, hi0 = int(off[0]), int(off[-1])
    assert same_bits(gk[:lo0], keys[:lo0]) and same_bits(gk[hi0:], keys[hi0:])
    assert same_bits(gv[:lo0], vals[:lo0]) and same_bits(gv[hi0:], vals[hi0:])
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        ek, ev = expected_pairs(keys[lo:hi], vals[lo:hi])
        assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), f"({kb}, {vb}): segment {s} of length {hi - lo}"
    gpu.sort_segments_device_tensor(hk, off, values=hv)
    assert same_bits(gk, to_host(hk, key)) and same_bits(gv, to_host(hv, vdtype))


# ---- 4. many items ---------------------------------------------------------------------------------------------------------------

def test_many_long_items(gpu):
    import torch
    key = "uint16"
    wave_max, T = gpu.segments_limits(key)
    lengths = many_items_lengths(wave_max, T)
    assert long_count(lengths, T) == MANY_LONG > 1024                                                   # the tile scan crosses a chunk
    assert tile_count(lengths, T) > 8 * torch.cuda.get_device_properties(0).multi_processor_count       # a workgroup takes a second tile
    off, n = offsets_of(lengths)
    a = _random(n, key, 9)
    _sort_both_ways(gpu, a, off, key, 4, "many long items")


# ---- 5. degenerate tables --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["uint32", "float64"])
def test_degenerate_tables(gpu, key):
    wave_max, block_max = gpu.segments_limits(key)
    for i, (name, off, n) in enumerate(degenerate_tables(wave_max, block_max)):
        a = _random(n, key, 20 + i)
        tmp0, tmp1 = _sort_both_ways(gpu, a, off, key, 8 if i % 2 else 4, f"{key}, {name}")
        _check_tmp(tmp0, tmp1, off, block_max, name)


# ---- 6. invalid tables -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ob", [4, 8])
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("with_long", [False, True])
def test_invalid_tables_change_nothing_and_are_reported(gpu, ob, pairs, with_long):
    key, vb = ("uint64", 4) if pairs else ("float32", 0)
    wave_max, block_max = gpu.segments_limits(key, vb)
    off, n = offsets_of([3, 2 * block_max + 5 if with_long else 900, 40, wave_max + 1, 2, block_max + 1 if with_long else 700, 6])
    gpu.device_status()
    for name, bad, bad_n in invalid_tables(off, n):
        size = n + 1
        k0, v0 = _random(size, key, 62), position_values(size, "uint32")
        tmpk0, tmpv0 = _random(size, key, 63), position_values(size, "uint32")[::-1].copy()
        tk, tv, ttk, ttv = to_device(k0), to_device(v0), to_device(tmpk0), to_device(tmpv0)
        gpu.sort_segments_device_offsets_nowait_tensor(tk[:bad_n], _torch_offsets(bad, ob), tmp=ttk[:bad_n], values=tv[:bad_n] if pairs else None,
                                                       tmp_values=ttv[:bad_n] if pairs else None, check=False)
        _table_error(gpu)
        gpu.device_status()                                   # reported once
        assert same_bits(to_host(tk, key), k0), name
        assert same_bits(to_host(tv, "uint32"), v0), name
        assert same_bits(to_host(ttk, key), tmpk0) and same_bits(to_host(ttv, "uint32"), tmpv0), name
    # a valid call afterwards sorts
    a = _random(n, key, 64)
    tk, tv = to_device(a), to_device(position_values(n, "uint32"))
    gpu.sort_segments_device_offsets_nowait_tensor(tk, _torch_offsets(off, ob), values=tv if pairs else None)
    check_segments(to_host(tk, key), a, off, key, "after the invalid tables")


# ---- 7. bounds -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ob", [4, 8])
def test_nothing_outside_the_buffers_is_written(gpu, ob):
    from rdst_amd import _lib
    from rdst_amd.radix_sort import key_info
    import torch
    key, vdtype = "int32", "uint64"
    kind, nbytes, levels = key_info(key)
    wave_max, block_max = gpu.segments_limits(key, 8)
    lengths = [5, block_max + 1, wave_max, 0, 2 * block_max + 17, block_max, 1, 3 * block_max]
    off, n = offsets_of(lengths)
    keys = _random(n, key, 71)
    vals = position_values(n, vdtype)
    tmpk0, tmpv0 = _random(n, key, 72), position_values(n, vdtype)[::-1].copy()
    table = np.ascontiguousarray(off, dtype=np.int32 if ob == 4 else np.int64)
    need = gpu.segments_nowait_scratch_bytes(len(off) - 1, n, key, 8)
    assert need > gpu.segments_device_offsets_scratch_bytes(len(off) - 1)
    bands = {"keys": Bands([("keys", keys, 4)], seed=1), "vals": Bands([("vals", vals, 8)], seed=2),
             "offsets": Bands([("offsets", table, 4 if ob == 4 else 8)], seed=3),            # 4-byte offsets: aligned to 4 bytes only
             "scratch": Bands([("scratch", ((need,), "uint8"), 0)], seed=4),
             "tmp": Bands([("tmp", tmpk0, 12)], seed=5), "tmpv": Bands([("tmpv", tmpv0, 8)], seed=6)}
    assert bands["scratch"]["scratch"].data_ptr() % 256 == 0
    vp = ctypes.c_void_p
    ptr = lambda name: vp(bands[name][name].data_ptr())   # noqa: E731
    s = vp(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    what = f"{ob}-byte offsets"
    _lib.check(lib.rdst_hip_sort_segments_pairs_device_offsets_nowait(ptr("keys"), ptr("vals"), ptr("tmp"), ptr("tmpv"), n, ptr("offsets"), ob,
                                                                      len(off) - 1, nbytes, kind, levels, 8, ptr("scratch"), need, s))
    gpu.device_status()
    gk, gv = to_host(bands["keys"]["keys"], key), to_host(bands["vals"]["vals"], vdtype)
    for sgm in range(len(off) - 1):
        lo, hi = int(off[sgm]), int(off[sgm + 1])
        ek, ev = expected_pairs(keys[lo:hi], vals[lo:hi])
        assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), f"{what}: segment {sgm}"
    lo0, hi0 = int(off[0]), int(off[-1])
    assert same_bits(gk[:lo0], keys[:lo0]) and same_bits(gk[hi0:], keys[hi0:]) and same_bits(gv[:lo0], vals[:lo0]) and same_bits(gv[hi0:], vals[hi0:])
    _check_tmp(tmpk0, to_host(bands["tmp"]["tmp"], key), off, block_max, what + ", tmp keys")
    _check_tmp(tmpv0, to_host(bands["tmpv"]["tmpv"], vdtype), off, block_max, what + ", tmp values")
    for name, b in bands.items():
        b.check(f"{what}: {name}", untouched=("offsets",) if name == "offsets" else ())
    # keys only, through the same buffers (the key-only tile is twice the pairs' one: other tiles, the same table)
    kb2 = Bands([("keys", keys, 4)], seed=7)
    need2 = gpu.segments_nowait_scratch_bytes(len(off) - 1, n, key)
    assert need2 <= need
    _lib.check(lib.rdst_hip_sort_segments_device_offsets_nowait(vp(kb2["keys"].data_ptr()), ptr("tmp"), n, ptr("offsets"), ob, len(off) - 1, nbytes, kind,
                                                                levels, ptr("scratch"), need2, s))
    gpu.device_status()
    check_segments(to_host(kb2["keys"], key), keys, off, key, what + " (keys only)")
    kb2.check(what + " (keys only)")
    for name in ("offsets", "scratch", "tmp"):
        bands[name].check(f"{what} (keys only): {name}", untouched=("offsets",) if name == "offsets" else ())


# ---- 8. streams ------------------------------------------------------------------------------------------------------------------

def test_offsets_from_a_cumsum_on_another_stream(gpu):
    import torch
    key = "uint32"
    wave_max, T = gpu.segments_limits(key)
    rng = np.random.default_rng(81)
    lengths = rng.integers(0, 41, size=2001)
    lengths[rng.choice(2001, size=8, replace=False)] = [T + 1, 2 * T + 9, wave_max + 1, T, 3 * T - 1, 600, T + 77, 0]
    n = int(lengths.sum()) + TAIL_GAP
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    a = _random(n, key, 82)
    t = to_device(a)
    tlen = torch.from_numpy(lengths).cuda()
    tmp = torch.empty_like(t)
    scratch = torch.empty(gpu.segments_nowait_scratch_bytes(len(lengths), n, key), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        toff = torch.zeros(len(lengths) + 1, dtype=torch.int64, device="cuda")
        toff[1:] = torch.cumsum(tlen, 0)                                       # queued on the stream; nothing comes to the host
        gpu.sort_segments_device_offsets_nowait_tensor(t, toff, tmp=tmp, scratch=scratch, check=False)
        gpu.device_status()
    torch.cuda.synchronize()
    check_segments(to_host(t, key), a, off, key, "cumsum on another stream")


# ---- the profiled run ---------------------------------------------------------------------------------------------------------------

def test_tiled_launches_are_one_stage_of_the_profiled_run(gpu):
    from rdst_amd import _lib
    key = "uint32"
    wave_max, T = gpu.segments_limits(key)
    off, n = offsets_of([7, T + 1, wave_max + 1])
    t = to_device(_random(n, key, 91))
    gpu.set_profiling(True)
    try:
        gpu.sort_segments_device_offsets_nowait_tensor(t, _torch_offsets(off, 8))
        lib = _lib.load()
        codes = []
        for run in range(gpu.profile_runs()):
            kinds, ms = (ctypes.c_uint32 * 64)(), (ctypes.c_float * 64)()
            nk, nm = ctypes.c_uint32(0), ctypes.c_uint32(0)
            _lib.check(lib.rdst_hip_profile_run(run, ms, 64, ctypes.byref(nm)))
            _lib.check(lib.rdst_hip_profile_run_stages(run, kinds, 64, ctypes.byref(nk)))
            assert nk.value == nm.value
            codes.append([int(kinds[i]) & 0xFF for i in range(nk.value)])
    finally:
        gpu.set_profiling(False)
    # the plan's pair sort records its own run first; then the call's: the counted launches, and the tiled launches as one stage
    assert codes and codes[-1] == [_lib.RDST_STAGE_SEGMENTS, _lib.RDST_STAGE_SEGMENTS_TILED], codes
    assert all(_lib.RDST_STAGE_SEGMENTS_TILED not in c for c in codes[:-1])
