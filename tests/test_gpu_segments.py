"""The segmented sort on the device (rdst_hip_sort_segments_device / _pairs_device; rdst_amd.sort_segments_device_tensor):
every segment must end exactly as the slice entry would leave it, whatever class serves it — one wave, one workgroup or
the whole-slice route — and nothing outside the segments may change.  Every length comes from segments_limits."""
import ctypes

import numpy as np
import pytest

from helpers import (DTYPES, PAIR_WIDTHS, SMALL_DTYPES, Bands, expected_pairs, key_dtype, poison_pattern, position_values, random_bits,
                     reference_sorted, same_bits, to_device, to_host, uint_view, unmapped, without_poison)
from test_gpu_bounds import MIXED

pytestmark = pytest.mark.gpu

HEAD_GAP, TAIL_GAP = 5, 7
WAVES_PER_WORKGROUP = 4   # SEG_WAVES of rdst_segments.hip: wave-class segments that share a workgroup
KEYS = DTYPES + SMALL_DTYPES + ("u128",)


def _np_dtype(key):
    return "uint64" if key == "u128" else key


def _ref(a, key):
    if key == "u128":
        return a[np.lexsort((a[:, 0], a[:, 1]))]
    return reference_sorted(a)


def _random(n, key, seed):
    if key == "u128":
        return random_bits(2 * n, "uint64", seed).reshape(n, 2).copy()
    return random_bits(n, key, seed).copy()


def _largest(key):
    """the key whose mapped image is all ones: what the kernels pad with"""
    if key == "u128":
        return np.full((1, 2), np.iinfo(np.uint64).max, dtype=np.uint64)
    dt = np.dtype(key)
    return unmapped(np.array([(1 << (8 * dt.itemsize)) - 1], dtype=f"u{dt.itemsize}"), key)


def edges_offsets(wave_max, block_max, seed=11, with_long=True):
    """EDGES: the lengths at which the classes and their kernels change, in a seeded shuffle, with a head gap and a tail gap
    and an empty segment at the very end; returns (offsets, n)"""
    lengths = [0, 0, 1, 2, 3, 63, 64, 65, wave_max - 1, wave_max, wave_max + 1, 1023, 1024, 1025, block_max - 1, block_max,
               block_max + 1, 2 * block_max + 17]
    if not with_long:
        lengths = [x for x in lengths if x <= block_max]
    lengths = list(np.random.default_rng(seed).permutation(lengths)) + [0]
    off = HEAD_GAP + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return off, int(off[-1]) + TAIL_GAP


def fill_segments(a, off, key, few=None):
    """per segment, in turn: random bits (as they are in `a`), already sorted, all equal, random with the last three
    elements set to the largest mapped key.  Float keys: the first random segment of at least eight keys starts with
    +-0, +-inf and NaNs of both signs.  `few`: keep only that many distinct values per random segment (ties)."""
    specials_done = False
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        if hi - lo == 0:
            continue
        seg = a[lo:hi]
        if few:
            pool = seg[:few].copy()
            seg[:] = pool[np.random.default_rng(s).integers(0, len(pool), size=hi - lo)]
        mode = s % 4
        if mode == 1:
            seg[:] = _ref(seg.copy(), key)
        elif mode == 2:
            seg[:] = seg[:1]
        elif mode == 3:
            seg[-3:] = _largest(key)
        elif key in ("float32", "float64") and hi - lo >= 8 and not specials_done:
            nan = np.array([np.nan], dtype=key)
            neg_nan = (uint_view(nan) | uint_view(np.array([-0.0], dtype=key))).view(key)
            seg[:6] = np.array([0.0, -0.0, np.inf, -np.inf, nan[0], neg_nan[0]], dtype=key)
            specials_done = True
    return a


def check_segments(got, orig, off, key, what=""):
    """every segment in the reference order, everything outside the segments as it was"""
    lo0, hi0 = int(off[0]), int(off[-1])
    assert same_bits(got[:lo0], orig[:lo0]) and same_bits(got[hi0:], orig[hi0:]), f"{what}: the gaps changed"
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        assert same_bits(got[lo:hi], _ref(orig[lo:hi], key)), f"{what}: segment {s} [{lo}, {hi}) of length {hi - lo}"


def edges_input(gpu, key, val_bytes=0, seed=3):
    wave_max, block_max = gpu.segments_limits(key, val_bytes)
    off, n = edges_offsets(wave_max, block_max)
    return fill_segments(_random(n, key, seed), off, key), off, n


@pytest.mark.parametrize("key", KEYS)
def test_parity_with_the_slice_entry(gpu, key):
    a, off, n = edges_input(gpu, key)
    wide = "u128" if key == "u128" else None
    items, counts, tmp_elems = gpu.segments_plan(off, n, key)
    wave_max, block_max = gpu.segments_limits(key)
    assert counts == (7, 6, 2) and tmp_elems == 2 * block_max + 17 and len(items) == 15
    t = to_device(a)
    gpu.sort_segments_device_tensor(t, off, check=False, key=wide)
    gpu.device_status()
    got = to_host(t, _np_dtype(key))
    check_segments(got, a, off, key, key)
    # the same input through a loop of the slice entry: the same bytes
    t2 = to_device(a)
    for s in range(len(off) - 1):
        gpu.sort_device_tensor(t2[int(off[s]):int(off[s + 1])], check=False, key=wide)
    gpu.device_status()
    assert same_bits(to_host(t2, _np_dtype(key)), got)
    # offsets as a numpy array, a list and a device tensor are the same call
    import torch
    for form in (list(int(x) for x in off), torch.from_numpy(off).cuda()):
        t3 = to_device(a)
        gpu.sort_segments_device_tensor(t3, form, key=wide)
        assert same_bits(to_host(t3, _np_dtype(key)), got)


@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_pairs_are_stable(gpu, kb, vb):
    key = key_dtype(kb, {(4, 4): "u", (4, 8): "i", (8, 4): "f", (8, 8): "u"}[(kb, vb)])
    vdtype = f"uint{8 * vb}"
    wave_max, block_max = gpu.segments_limits(key, vb)
    off, n = edges_offsets(wave_max, block_max)
    keys = fill_segments(_random(n, key, 5), off, key, few=3)    # three distinct keys per segment at most: ties everywhere
    vals = position_values(n, vdtype)
    tk, tv = to_device(keys), to_device(vals)
    gpu.sort_segments_device_tensor(tk, off, values=tv, check=False)
    gpu.device_status()
    gk, gv = to_host(tk, key), to_host(tv, vdtype)
    lo0, hi0 = int(off[0]), int(off[-1])
    assert same_bits(gk[:lo0], keys[:lo0]) and same_bits(gk[hi0:], keys[hi0:])
    assert same_bits(gv[:lo0], vals[:lo0]) and same_bits(gv[hi0:], vals[hi0:])
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        ek, ev = expected_pairs(keys[lo:hi], vals[lo:hi])
        assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), f"({kb}, {vb}) segment {s} of length {hi - lo}"


def _tiny_offsets(gpu, key, val_bytes, nseg=20_000, seed=21):
    lengths = np.random.default_rng(seed).integers(0, 41, size=nseg)
    j = 0
    while int((lengths >= 2).sum()) % WAVES_PER_WORKGROUP != 1:    # the last workgroup holds one segment and three idle waves
        if lengths[j] >= 2:
            lengths[j] = 0
        j += 1
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64) + HEAD_GAP
    return off, int(off[-1]) + TAIL_GAP


def test_many_tiny_segments(gpu):
    off, n = _tiny_offsets(gpu, "uint32", 0)
    _items, counts, tmp_elems = gpu.segments_plan(off, n, "uint32")
    assert counts[1] == counts[2] == 0 and tmp_elems == 0
    assert counts[0] % WAVES_PER_WORKGROUP != 0 and counts[0] // WAVES_PER_WORKGROUP > 4 * 256    # a partly filled last workgroup; a grid beyond the device
    for key in ("uint32", "float64"):
        a = fill_segments(_random(n, key, 8), off, key)
        t = to_device(a)
        gpu.sort_segments_device_tensor(t, off)
        check_segments(to_host(t, key), a, off, key, key)
    keys = random_bits(n, "uint32", 9) & np.uint32(3)
    vals = position_values(n, "uint64")
    tk, tv = to_device(keys), to_device(vals)
    gpu.sort_segments_device_tensor(tk, off, values=tv)
    gk, gv = to_host(tk, "uint32"), to_host(tv, "uint64")
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        ek, ev = expected_pairs(keys[lo:hi], vals[lo:hi])
        assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), s
    assert same_bits(gv[int(off[-1]):], vals[int(off[-1]):]) and same_bits(gv[:HEAD_GAP], vals[:HEAD_GAP])


def test_many_block_class_segments(gpu):
    lengths = np.random.default_rng(31).integers(2000, 4001, size=600)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64) + HEAD_GAP
    n = int(off[-1]) + TAIL_GAP
    for key, vb in (("uint32", 0), ("int64", 0), ("uint64", 8)):
        _items, counts, _tmp = gpu.segments_plan(off, n, key, vb)
        assert counts == (0, 600, 0)      # 600 workgroups of 1 024 threads: more than can be resident at once
        a = fill_segments(_random(n, key, 12), off, key)
        t = to_device(a)
        if vb == 0:
            gpu.sort_segments_device_tensor(t, off)
            check_segments(to_host(t, key), a, off, key, key)
        else:
            a &= np.uint64(7)
            t = to_device(a)
            vals = position_values(n, "uint64")
            tv = to_device(vals)
            gpu.sort_segments_device_tensor(t, off, values=tv)
            gk, gv = to_host(t, key), to_host(tv, "uint64")
            for s in range(600):
                lo, hi = int(off[s]), int(off[s + 1])
                ek, ev = expected_pairs(a[lo:hi], vals[lo:hi])
                assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), s


def _abi_call(gpu, keys, tmp, tmp_elems, n, off, key, values=None, tmp_values=None):
    """the entries themselves, with exactly the pointers and sizes given (tmp may be None)"""
    import torch
    from rdst_amd import _lib
    from rdst_amd.radix_sort import key_info
    kind, nbytes, levels = key_info(key)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    offp = o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    vp = ctypes.c_void_p
    ptr = lambda t: vp(t.data_ptr() if t is not None else None)   # noqa: E731
    s = vp(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    if values is None:
        _lib.check(lib.rdst_hip_sort_segments_device(ptr(keys), ptr(tmp), tmp_elems, n, offp, len(o) - 1, nbytes, kind, levels, s))
    else:
        _lib.check(lib.rdst_hip_sort_segments_pairs_device(ptr(keys), ptr(values), ptr(tmp), ptr(tmp_values), tmp_elems, n, offp, len(o) - 1,
                                                           nbytes, kind, levels, values.element_size(), s))


@pytest.mark.parametrize("fill", ["random", "poison"])
@pytest.mark.parametrize("key", ["uint8", "int16", "float32", "uint64", "u128"])
def test_placement_keys(gpu, key, fill):
    nb = 16 if key == "u128" else np.dtype(key).itemsize
    koff, toff = MIXED[nb]
    pat = poison_pattern(key) if fill == "poison" else "random"
    a, off, n = edges_input(gpu, key, seed=17)
    if fill == "poison":
        a = without_poison(a, key)
    _wave_max, block_max = gpu.segments_limits(key)
    longest = 2 * block_max + 17
    kb = Bands([("keys", a, koff)], seed=1, fill=pat)
    tb = Bands([("tmp", ((longest,) + a.shape[1:], a.dtype), toff)], seed=2, fill=pat)
    _abi_call(gpu, kb["keys"], tb["tmp"], longest, n, off, key)
    gpu.device_status()
    what = f"{key} fill={fill}"
    check_segments(to_host(kb["keys"], _np_dtype(key)), a, off, key, what)
    kb.check(what)
    tb.check(what)
    # no long segment: a NULL tmp is accepted
    short, n_short = edges_offsets(_wave_max, block_max, with_long=False)
    assert n_short <= n and gpu.segments_plan(short, n, key)[1][2] == 0
    kb2 = Bands([("keys", a, koff)], seed=3, fill=pat)
    _abi_call(gpu, kb2["keys"], None, 0, n, short, key)
    gpu.device_status()
    got = to_host(kb2["keys"], _np_dtype(key))
    check_segments(got, a, short, key, what + " (no tmp)")
    kb2.check(what + " (no tmp)")


@pytest.mark.parametrize("fill", ["random", "poison"])
@pytest.mark.parametrize("kb_,vb", [(4, 8), (8, 4)])
def test_placement_pairs(gpu, kb_, vb, fill):
    key, vdtype = key_dtype(kb_, "i"), f"uint{8 * vb}"
    pat = poison_pattern(key) if fill == "poison" else "random"
    wave_max, block_max = gpu.segments_limits(key, vb)
    off, n = edges_offsets(wave_max, block_max)
    keys = fill_segments(_random(n, key, 19), off, key)
    if fill == "poison":
        keys = without_poison(keys, key)
    vals = position_values(n, vdtype)
    longest = 2 * block_max + 17
    (koff, toff), (voff, tvoff) = MIXED[kb_], MIXED[vb]
    what = f"({kb_}, {vb}) fill={fill}"
    bands = {"keys": Bands([("keys", keys, koff)], seed=4, fill=pat), "vals": Bands([("vals", vals, voff)], seed=5, fill=pat),
             "tmp": Bands([("tmp", ((longest,), keys.dtype), toff)], seed=6, fill=pat),
             "tmpv": Bands([("tmpv", ((longest,), vals.dtype), tvoff)], seed=7, fill=pat)}
    _abi_call(gpu, bands["keys"]["keys"], bands["tmp"]["tmp"], longest, n, off, key, values=bands["vals"]["vals"], tmp_values=bands["tmpv"]["tmpv"])
    gpu.device_status()
    gk, gv = to_host(bands["keys"]["keys"], key), to_host(bands["vals"]["vals"], vdtype)
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        ek, ev = expected_pairs(keys[lo:hi], vals[lo:hi])
        assert same_bits(gk[lo:hi], ek) and same_bits(gv[lo:hi], ev), f"{what} segment {s}"
    lo0, hi0 = int(off[0]), int(off[-1])
    assert same_bits(gv[:lo0], vals[:lo0]) and same_bits(gv[hi0:], vals[hi0:]) and same_bits(gk[:lo0], keys[:lo0]) and same_bits(gk[hi0:], keys[hi0:])
    for b in bands.values():
        b.check(what)


def test_other_stream_right_after_a_whole_slice_sort(gpu):
    """the workspace changes hands between streams: a whole-slice sort queued on the default stream, the segmented sort
    directly behind it on another one"""
    import torch
    a, off, n = edges_input(gpu, "uint32", seed=23)
    big = random_bits(1 << 21, "uint64", 24)
    t, tb = to_device(a), to_device(big)
    tmp_big = torch.empty_like(tb)
    torch.cuda.synchronize()
    other = torch.cuda.Stream()
    gpu.sort_device_tensor(tb, tmp_big, check=False)
    with torch.cuda.stream(other):
        gpu.sort_segments_device_tensor(t, off, check=False)
    torch.cuda.synchronize()
    gpu.device_status()
    with torch.cuda.stream(other):
        gpu.device_status()
    assert same_bits(to_host(tb, "uint64"), reference_sorted(big))
    check_segments(to_host(t, "uint32"), a, off, "uint32", "other stream")


def test_profiling_lists_the_segments_stage(gpu):
    from rdst_amd import _lib
    a, off, n = edges_input(gpu, "uint32", seed=29)
    t = to_device(a)
    gpu.set_profiling(True)
    try:
        gpu.sort_segments_device_tensor(t, off)
        lib = _lib.load()
        codes = []
        for run in range(gpu.profile_runs()):
            kinds = (ctypes.c_uint32 * 64)()
            ms = (ctypes.c_float * 64)()
            nk, nm = ctypes.c_uint32(0), ctypes.c_uint32(0)
            _lib.check(lib.rdst_hip_profile_run(run, ms, 64, ctypes.byref(nm)))
            _lib.check(lib.rdst_hip_profile_run_stages(run, kinds, 64, ctypes.byref(nk)))
            assert nk.value == nm.value
            codes.append([int(kinds[i]) & 0xFF for i in range(nk.value)])
    finally:
        gpu.set_profiling(False)
    assert codes and codes[0] == [_lib.RDST_STAGE_SEGMENTS]         # the batched launches: one run, one stage
    assert len(codes) == 3                                          # and a run for each of the two long segments, as ever
    assert all(_lib.RDST_STAGE_SEGMENTS not in c for c in codes[1:])
    check_segments(to_host(t, "uint32"), a, off, "uint32", "profiling")
