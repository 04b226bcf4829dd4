"""The key-value sort (rdst_hip_sort_pairs_device) at the pass shapes and skips that only pairs take: tiles of 8 448, 5 376
and 3 840 pairs, values staged next to the keys, every tile ranked by the ballots or the careful path, values copied back
after an odd number of passes.  Every case: values that name their position (position_values), the result compared with THE
stable order of the mapped keys (expected_pairs), then the device's status word.  tests/test_pairs_inputs.py checks, without
a device, that each input is what its name says."""
import numpy as np
import pytest

from helpers import (COPY_BACK_LEVELS, PAIR_WIDTHS, banded, chain_split_cases, constant_level_inputs, constant_levels, copy_back_inputs,
                     expected_pairs, increasing_mapped, key_dtype, mapped_key, mask_other_bytes, pair_heavy_digit_inputs, pair_kpt, pair_lengths,
                     pair_tile, position_values, random_bits, same_bits, to_device, to_host, uint_view, value_positions)

pytestmark = pytest.mark.gpu
KINDS = ("u", "i", "f")


def _vdtype(vb):
    return f"int{8 * vb}"


def _check(gpu, keys, vb, what, expected=None):
    """sort (keys, position values) on the device and compare both arrays with the stable order of the mapped keys"""
    vals = position_values(len(keys), _vdtype(vb))
    ek, ev = expected if expected is not None else expected_pairs(keys, vals)
    tk, tv = to_device(keys), to_device(vals)
    gpu.sort_pairs_device_tensor(tk, tv)
    gk, gv = to_host(tk, keys.dtype), to_host(tv, vals.dtype)
    assert same_bits(gk, ek), ("keys", what, _first_difference(uint_view(gk), uint_view(ek)))
    assert np.array_equal(gv, ev), ("values", what, _first_difference(gv, ev))
    gpu.device_status()
    return gk, gv


def _first_difference(a, b):
    d = np.flatnonzero(a != b)
    return f"{d.size} differ, first at {int(d[0])} of {len(a)}" if d.size else "equal"


# ---- a. pass parity and skipped levels ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_skipped_levels_carry_the_values(gpu, kb, vb, kind):
    """Constant levels are skipped: the values ping-pong with the keys (src_is_tmp), the first executed level may lie above 0,
    a pass after a skipped level runs on one chain, and an odd number of passes ends in tmp — keys AND values are copied
    back.  The parity of the passes left decides whether copyback_kernel<V> moves data."""
    try:
        for name, _levels, passes, keys in constant_level_inputs(kb, vb, kind):
            _check(gpu, keys, vb, (kb, vb, kind, name, f"{passes} passes"))
    finally:
        gpu.set_tuning()


# ---- b. the forms of the copy-back ---------------------------------------------------------------------------------------------

def _placements(kb, vb):
    """byte offsets from a 16-byte boundary of (keys, values, tmp keys, tmp values)"""
    koff = [o for o in (4, 8, 12) if o % kb == 0]
    voff = [o for o in (4, 8, 12) if o % vb == 0]
    out = [("all aligned", (0, 0, 0, 0))]
    out += [(f"values at +{o}", (0, o, 0, 0)) for o in voff]
    out += [(f"only tmp values at +{o}", (0, 0, 0, o)) for o in voff]
    out += [(f"keys at +{o}, values aligned", (o, 0, 0, 0)) for o in koff]
    out += [(f"only tmp keys at +{koff[-1]}", (0, 0, koff[-1], 0)), ("all four unaligned", (koff[0], voff[-1], koff[-1], voff[0]))]
    return out


@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_copy_back_forms(gpu, kb, vb):
    """An odd number of passes (level 1 constant, at every length) leaves the result in the tmps.  copyback_kernel copies
    16-byte vectors where both of its pointers allow them and single elements elsewhere, and its first block copies what is left behind the last
    whole vector: buffers at every element-aligned offset from a 16-byte boundary, lengths with every remainder of
    n * sizeof(V) modulo 16 (so the vector body and the tail both carry data), the bytes around each buffer unchanged."""
    dtype, vdt = key_dtype(kb, "u"), _vdtype(vb)
    remainders = set()
    try:
        for keys in copy_back_inputs(kb, vb):
            assert constant_levels(keys) == COPY_BACK_LEVELS and (kb - len(COPY_BACK_LEVELS)) % 2 == 1   # ends in the tmps
            n = len(keys)
            remainders.add(n * vb % 16)
            vals = position_values(n, vdt)
            ek, ev = expected_pairs(keys, vals)
            for place, (ko, vo, tko, tvo) in _placements(kb, vb):
                bk = banded(n, dtype, ko, band_bytes=4096, seed=1, init=keys)
                bv = banded(n, vdt, vo, band_bytes=4096, seed=2, init=vals)
                btk = banded(n, dtype, tko, band_bytes=4096, seed=3)
                btv = banded(n, vdt, tvo, band_bytes=4096, seed=4)
                views = (bk["keys"], bv["keys"], btk["keys"], btv["keys"])
                assert [t.data_ptr() % 16 for t in views] == [ko, vo, tko, tvo]
                gpu.sort_pairs_device_tensor(views[0], views[1], views[2], views[3])
                gk, gv = to_host(views[0], dtype), to_host(views[1], vdt)
                what = (kb, vb, n, place)
                assert same_bits(gk, ek), ("keys", what, _first_difference(gk, ek))
                assert np.array_equal(gv, ev), ("values", what, _first_difference(gv, ev))
                for b in (bk, bv, btk, btv):
                    b.check(str(what))
                gpu.device_status()
    finally:
        gpu.set_tuning()
    assert remainders == ({0, 4, 8, 12} if vb == 4 else {0, 8})


# ---- c. digit shapes on the careful ranking path --------------------------------------------------------------------------------

@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_heavy_digits_on_pair_tiles(gpu, kb, vb):
    """Pair tiles have no fast ranking: rounds of one digit are ranked by lane number (uniform_rounds), crowded digits by
    peers_below_total.  Every heavy-digit input at the levels 0, 1 and top — as it is (a misranked round shows as keys out of
    order on the lower bits) and with every other byte cut to two bits (many whole keys are equal: a misranked round shows in
    the order of the values alone)."""
    try:
        for name, level, a in pair_heavy_digit_inputs(kb, vb):
            _check(gpu, a, vb, (kb, vb, len(a), level, name))
            _check(gpu, mask_other_bytes(a, level), vb, (kb, vb, len(a), level, name, "other bytes masked"))
    finally:
        gpu.set_tuning()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_nearly_sorted_descending_and_few_values(gpu, kb, vb, kind):
    """Sorted keys with one swapped neighbour pair (the passes run, with almost every round of one digit) — at a round's, a
    wave's and a tile's border and inside the last, partial tile (the long length; the short one's last tile holds one pair, so
    its swap straddles that tile's border); strictly descending keys; keys of 3 distinct values."""
    dtype = key_dtype(kb, kind)
    kpt, tile = pair_kpt(kb, vb), pair_tile(kb, vb)
    try:
        for n in pair_lengths(kb, vb):
            base = increasing_mapped(n, dtype, seed=n)
            m = mapped_key(base)
            assert (m[1:] > m[:-1]).all()
            vals = position_values(n, _vdtype(vb))
            last = tile * (n // tile)
            for i in sorted({63, 64 * kpt - 1, tile - 1, (last + n - 1) // 2 if n - last >= 2 else last - 1}):
                a = base.copy()
                a[i], a[i + 1] = base[i + 1], base[i]
                order = np.arange(n)
                order[i], order[i + 1] = i + 1, i
                _check(gpu, a, vb, (dtype, vb, n, "swapped", i), expected=(base, vals[order]))
            _check(gpu, base[::-1].copy(), vb, (dtype, vb, n, "descending"), expected=(base, vals[::-1]))
            pool = random_bits(3, dtype, seed=3)
            assert len(np.unique(uint_view(pool))) == 3
            three = pool[np.random.default_rng(n).integers(0, 3, size=n)]
            _check(gpu, three, vb, (dtype, vb, n, "3 distinct values"))
    finally:
        gpu.set_tuning()


# ---- d. chain-split shapes at pair tiles ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_chain_split_shapes_at_pair_tiles(gpu, kb, vb):
    """The case table of test_chain_split_shapes with the segment arithmetic of scan_kernel at pair tile sizes: several
    tiles on every chain, `short` with every segment below one tile, `tiny` below one tile in all; split on and off; and the
    ranking knobs, which no pairs result may depend on (pair tiles have no fast ranking)."""
    tile = pair_tile(kb, vb)
    dtype = key_dtype(kb, "u")
    cases = chain_split_cases(pair_lengths(kb, vb)[1], dtype, short=8 * tile - 5, tiny=700)
    assert len(cases["short"]) == 8 * tile - 5 and len(cases["tiny"]) == 700
    try:
        for name, a in cases.items():
            a = np.ascontiguousarray(a).view(dtype)
            exp = expected_pairs(a, position_values(len(a), _vdtype(vb)))
            for split in (True, False):
                gpu.set_tuning(chain_split=split)
                _check(gpu, a, vb, (kb, vb, name, "chain_split", split), expected=exp)
            if name == "uniform":
                for fast in (0, 2):
                    gpu.set_tuning(fast_rank=fast)
                    _check(gpu, a, vb, (kb, vb, name, "fast_rank", fast), expected=exp)
    finally:
        gpu.set_tuning()


# ---- e. lengths -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_lengths_around_rounds_waves_and_tiles(gpu, kb, vb, kind):
    """Keys of 5 distinct values: with values that name their position, every length checks the stability of the partial
    tile (and of a partial round, and of a partial wave)."""
    dtype = key_dtype(kb, kind)
    kpt, t = pair_kpt(kb, vb), pair_tile(kb, vb)
    five = random_bits(5, dtype, seed=55)
    assert len(np.unique(mapped_key(five))) == 5
    try:
        for n in (2, 3, 63, 64, 65, 64 * kpt - 1, 64 * kpt + 1, t - 1, t, t + 1, 8 * t - 1, 8 * t, 8 * t + 1, 9 * t + 1):
            keys = five[np.random.default_rng(n).integers(0, 5, size=n)]
            if n == 2:
                keys = five[[3, 1]] if mapped_key(five)[3] > mapped_key(five)[1] else five[[1, 3]]   # the one inversion
            _check(gpu, keys, vb, (dtype, vb, n))
    finally:
        gpu.set_tuning()


# ---- f. float specials as keys --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vb", [4, 8])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_specials_as_keys(gpu, dtype, vb):
    ut = f"u{np.dtype(dtype).itemsize}"
    w = 8 * np.dtype(dtype).itemsize
    mant = 23 if w == 32 else 52
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1e30, -1e30,
                   np.finfo(dtype).max, -np.finfo(dtype).max, np.finfo(dtype).tiny, -np.finfo(dtype).tiny,               # normals
                   np.finfo(dtype).smallest_subnormal, -np.finfo(dtype).smallest_subnormal,                             # denormals
                   np.finfo(dtype).tiny / 2, -np.finfo(dtype).tiny / 2], dtype=dtype)
    exp_all = ((1 << (w - 1)) - 1) & ~((1 << mant) - 1)                  # the exponent field, all ones
    payloads = [1, 2, 1 << (mant - 1), (1 << mant) - 1]                  # signalling NaNs, np.nan's own pattern, every bit set
    nans = np.array([s | exp_all | p for s in (0, 1 << (w - 1)) for p in payloads], dtype=ut).view(dtype)
    assert np.isnan(nans).all()
    pool = np.concatenate((sp, nans))
    assert len(np.unique(uint_view(pool))) == len(pool)
    a = np.tile(pool, 700)
    np.random.default_rng(6).shuffle(a)
    try:
        gk, gv = _check(gpu, a, vb, (dtype, vb))
    finally:
        gpu.set_tuning()
    bits = uint_view(gk)
    minus0, plus0 = np.flatnonzero(bits == 1 << (w - 1)), np.flatnonzero(bits == 0)
    assert len(minus0) == len(plus0) == 700 and minus0.max() < plus0.min()               # -0.0 sorts before +0.0
    assert np.isnan(gk[0]) and np.signbit(gk[0]) and np.isnan(gk[-1]) and not np.signbit(gk[-1])
    came_from = value_positions(gv)
    assert same_bits(a[came_from], gk)                                                    # every value still names its key
    same = bits[1:] == bits[:-1]
    assert same.sum() == len(a) - len(pool) and (came_from[1:][same] > came_from[:-1][same]).all()   # equal bits keep their order


# ---- g. streams and the workspace -----------------------------------------------------------------------------------------------

def test_pair_sorts_and_a_key_sort_share_the_workspace_on_two_streams(gpu):
    import torch
    n1, n2 = pair_lengths(4, 8)[1], pair_lengths(8, 4)[1]
    k1, k2, k3 = random_bits(n1, "float32", seed=31).copy(), random_bits(n2, "int64", seed=32).copy(), random_bits(300_001, "uint32", seed=33).copy()
    k1 = mask_other_bytes(k1, 3)                 # equal keys: the value order counts
    v1, v2 = position_values(n1, "int64"), position_values(n2, "int32")
    e1, e2 = expected_pairs(k1, v1), expected_pairs(k2, v2)
    tk1, tv1, tk2, tv2, t3 = to_device(k1), to_device(v1), to_device(k2), to_device(v2), to_device(k3)
    tmps = [torch.empty_like(t) for t in (tk1, tv1, tk2, tv2, t3)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):                  # two pair sorts of different widths back to back, no sync in between
        gpu.sort_pairs_device_tensor(tk1, tv1, tmps[0], tmps[1], check=False)
        gpu.sort_pairs_device_tensor(tk2, tv2, tmps[2], tmps[3], check=False)
    with torch.cuda.stream(s2):
        gpu.sort_device_tensor(t3, tmps[4], check=False)
    with torch.cuda.stream(s1):
        gpu.device_status()
    with torch.cuda.stream(s2):
        gpu.device_status()
    assert same_bits(to_host(tk1, "float32"), e1[0]) and np.array_equal(to_host(tv1, "int64"), e1[1])
    assert same_bits(to_host(tk2, "int64"), e2[0]) and np.array_equal(to_host(tv2, "int32"), e2[1])
    assert np.array_equal(to_host(t3, "uint32"), np.sort(k3))


# ---- h. the routes that ride on pairs, at a skipping key ---------------------------------------------------------------------------

def test_record_routes_with_skipped_levels(gpu):
    """sort_records_by_key on a float column of 200 small positive integers (the low mantissa bytes are constant: the pair
    sort of (key, row) skips levels), and the host records entry with an <i8 key that fits 3 bytes (five constant levels: an
    odd number of passes) — rows in the stable order of the mapped keys."""
    import torch
    rng = np.random.default_rng(8)
    n = pair_lengths(4, 4)[1]
    rec = rng.standard_normal((n, 3)).astype(np.float32)
    rec[:, 1] = rng.integers(1, 201, size=n).astype(np.float32)
    assert {0, 1} <= constant_levels(rec[:, 1].copy()) and len(np.unique(rec[:, 1])) == 200
    out = gpu.sort_records_by_key(torch.from_numpy(rec).cuda(), 1).cpu().numpy()
    order = np.argsort(mapped_key(rec[:, 1].copy()), kind="stable")
    assert np.array_equal(out.view(np.uint32), rec[order].view(np.uint32))
    gpu.device_status()

    rec_dt = np.dtype([("id", "<u4"), ("key", "<i8"), ("pad", "<u4")], align=True)
    n = pair_lengths(8, 4)[1]
    a = np.zeros(n, dtype=rec_dt)
    a.view(np.uint8).reshape(n, rec_dt.itemsize)[:] = rng.integers(0, 256, size=(n, rec_dt.itemsize), dtype=np.uint8)
    a["key"] = rng.integers(0, 1 << 24, size=n, dtype=np.int64)
    a["key"][::3] = a["key"][0]
    assert constant_levels(a["key"].copy()) == {3, 4, 5, 6, 7}
    order = np.argsort(mapped_key(a["key"].copy()), kind="stable")
    exp = a.view(np.uint8).reshape(n, rec_dt.itemsize)[order].copy()
    gpu.sort_host_records(a, "key")
    assert np.array_equal(a.view(np.uint8).reshape(n, rec_dt.itemsize), exp)
    gpu.device_status()
