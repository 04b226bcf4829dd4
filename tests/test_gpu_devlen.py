"""The sorts of a prefix whose length lives in device memory (rdst_hip_sort_device_devlen,
rdst_hip_sort_pairs_device_devlen) on the device: the first m elements end up bit for bit as the known-length
twins leave a slice of m elements, everything from m on — keys, values, both tmps — stays as it was, at every length at
which K1, K2, K3 or the copy-back change what they do; tails that would show if they were read; lengths past the capacity;
a length that a kernel is still computing when the call is made; buffers between guard bands."""
import numpy as np
import pytest

import devlen_inputs as D
import helpers as H

pytestmark = pytest.mark.gpu

RDST_ERR_DEVICE = -5
POISON = 0xA5


def _dev(a):
    return H.to_device(np.ascontiguousarray(a))


def _host(t, like):
    return H.to_host(t, like.dtype).reshape(like.shape)


def _poison(like):
    """a device tensor shaped like `like`, every byte POISON"""
    return _dev(np.full(like.nbytes, POISON, dtype=np.uint8).view(like.dtype).reshape(like.shape))


def _poisoned_from(t, like, m):
    """the elements of the tmp tensor `t` from m on still hold the poison"""
    return bool((_host(t, like)[m:].view(np.uint8) == POISON).all())


def _length(m, dtype):
    """a one-element device tensor of `dtype` whose bits are the low bits of m (read as unsigned by the library)"""
    import torch
    w = np.dtype(dtype).itemsize
    bits = np.array([m & ((1 << (8 * w)) - 1)], dtype=f"u{w}")
    return torch.from_numpy(bits.view(dtype).copy()).cuda()


def _with_equal_keys(a, seed):
    """a quarter of the keys drawn from a pool of 50: equal keys whose order the values tell"""
    rng = np.random.default_rng(seed)
    at = rng.choice(len(a), size=len(a) // 4, replace=False)
    a[at] = a[rng.integers(0, 50, size=at.size)]
    return a


def _sort_keys(gpu, a, m, key, length_dtype, tmp=None):
    """the device-length sort of `a` (numpy) at length m and the twin on a clone of the prefix: (result, tmp, twin's result)"""
    k = _dev(a)
    t = _poison(a) if tmp is None else tmp
    wide = "u128" if key == "u128" else None
    gpu.sort_device_devlen_tensor(k, _length(m, length_dtype), t, check=False, key=wide)
    k2 = _dev(a[:m])
    gpu.sort_device_tensor(k2, key=wide)
    gpu.device_status()
    return _host(k, a), t, _host(k2, a[:m])


def _check_keys(gpu, a, m, key, length_dtype, what):
    got, t, twin = _sort_keys(gpu, a, m, key, length_dtype)
    exp = D.expected_prefix_sorted(a, m)
    assert np.array_equal(got[:m].view(np.uint8), exp[:m].view(np.uint8)), what
    assert np.array_equal(got[:m].view(np.uint8), twin.view(np.uint8)), what
    assert np.array_equal(got[m:].view(np.uint8), a[m:].view(np.uint8)), f"{what}: the tail changed"
    assert _poisoned_from(t, a, m), f"{what}: tmp written from m on"
    return t


def _check_pairs(gpu, a, v, m, length_dtype, what):
    k, vv, tk, tv = _dev(a), _dev(v), _poison(a), _poison(v)
    gpu.sort_pairs_device_devlen_tensor(k, vv, _length(m, length_dtype), tk, tv, check=False)
    k2, v2 = _dev(a[:m]), _dev(v[:m])
    gpu.sort_pairs_device_tensor(k2, v2)
    gpu.device_status()
    gk, gv = _host(k, a), _host(vv, v)
    ek, ev = H.expected_pairs(a[:m], v[:m])
    assert H.same_bits(gk[:m], ek) and H.same_bits(gv[:m], ev), what
    assert H.same_bits(gk[:m], _host(k2, a[:m])) and H.same_bits(gv[:m], _host(v2, v[:m])), what
    assert H.same_bits(gk[m:], a[m:]) and H.same_bits(gv[m:], v[m:]), f"{what}: the tail changed"
    assert _poisoned_from(tk, a, m) and _poisoned_from(tv, v, m), f"{what}: a tmp written from m on"
    return tk, tv


# ---- 1: pairs, every width, at every border -------------------------------------------------------------------------

@pytest.mark.parametrize("kind,kb,vb", D.PAIR_CASES, ids=[f"{k}{8 * kb}-v{8 * vb}" for k, kb, vb in D.PAIR_CASES])
def test_pairs_prefix_at_every_border(gpu, kind, kb, vb):
    key, val = H.key_dtype(kb, kind), f"uint{8 * vb}"
    cap = D.pair_capacity(kb, vb)
    a = _with_equal_keys(H.random_bits(cap, key, 100 + kb + vb).copy(), kb * vb)
    v = H.position_values(cap, val)
    for i, (m, what) in enumerate(D.pair_lengths(kb, vb)):
        _check_pairs(gpu, a, v, m, D.LENGTH_DTYPES[i % 4], f"{key}/{val} m = {m} ({what})")


# ---- 2: keys only, every width, capacities on both sides of the one-workgroup tile -------------------------------------

@pytest.mark.parametrize("key,kb", D.KEY_CASES, ids=[k for k, _ in D.KEY_CASES])
def test_keys_prefix_at_every_border(gpu, key, kb):
    for cap in D.key_capacities(kb):
        a = D.random_keys(cap, key, cap + kb)
        for i, m in enumerate(D.small_lengths(cap)):
            _check_keys(gpu, a, m, key, D.LENGTH_DTYPES[(i + cap) % 4], f"{key} capacity {cap} m = {m}")
    a = D.random_keys(D.KEYS_CAPACITY, key, kb)
    for i, (m, what) in enumerate(D.key_lengths(key, kb)):
        _check_keys(gpu, a, m, key, D.LENGTH_DTYPES[i % 4], f"{key} m = {m} ({what})")
    gpu.sort_device_devlen_tensor(_dev(a), _length(len(a), "int64"), key="u128" if key == "u128" else None)
    assert gpu.last_route() == "lsd"


# ---- 3: a tail that would show if it were read -----------------------------------------------------------------------

@pytest.mark.parametrize("name", D.TAIL_FAMILIES)
def test_tail_is_never_read(gpu, name):
    # pairs (4, 4): three tiles of 8 448 and a few; keys only u64: three tiles of 10 752 and a few; m a multiple of nothing
    for pairs, key, tile in ((True, "uint32", H.pair_tile(4, 4)), (True, "float32", H.pair_tile(4, 4)), (False, "uint64", D.pass_tile(8, False)),
                             (False, "float64", D.pass_tile(8, True))):
        cap, m = 3 * tile + 11, 2 * tile - 345
        a = D.tail_case(name, cap, m, key)
        what = f"{name} {key} {'pairs' if pairs else 'keys'}"
        if pairs:
            v = H.position_values(cap, "uint32")
            tk, tv = _check_pairs(gpu, a, v, m, "int64", what)
            if name == "sorted prefix":          # nothing in any array changes: no pass ran, the tmps were never written
                assert _poisoned_from(tk, a, 0) and _poisoned_from(tv, v, 0), what
        else:
            got, t, _twin = _sort_keys(gpu, a, m, key, "uint32")
            exp = D.expected_prefix_sorted(a, m)
            assert H.same_bits(got, exp), what
            assert _poisoned_from(t, a, m if name != "sorted prefix" else 0), what
        if name == "sorted prefix":
            assert H.same_bits(D.expected_prefix_sorted(a, m), a)


@pytest.mark.parametrize("key,levels", D.NARROW_WIDE_TAILS, ids=[k for k, _ in D.NARROW_WIDE_TAILS])
@pytest.mark.parametrize("name", D.NARROW_WIDE_FAMILIES)
def test_tail_is_never_read_at_2_and_16_byte_keys(gpu, name, key, levels):
    """K2's trivial-level test must look at the first m keys only: a prefix that is constant at level 1 (int16) or at the
    levels 0 to 2 (u128) before a tail that varies there leaves an odd number of passes, so copyback_devlen_kernel moves
    exactly m keys; a sorted prefix before an unsorted tail runs no pass and writes nothing."""
    wide = key == "u128"
    kb = 16 if wide else np.dtype(key).itemsize
    tile = D.pass_tile(kb, not wide and np.dtype(key).kind != "u")
    cap, m = 3 * tile + 11, 2 * tile - 345
    a = D.tail_case_levels(name, cap, m, key, levels)
    what = f"{name} {key} keys"
    t = _check_keys(gpu, a, m, key, "uint32", what)
    if name == "sorted prefix":
        assert H.same_bits(D.expected_prefix_sorted(a, m), a)
        assert _poisoned_from(t, a, 0), f"{what}: tmp written"


# ---- 4: a length past the capacity -------------------------------------------------------------------------------------

PAST = (("capacity + 1", None, "int64"), ("2^32 - 1", (1 << 32) - 1, "uint32"), ("2^63", 1 << 63, "uint64"), ("2^63 in an int64", 1 << 63, "int64"),
        ("-1 in an int32", -1, "int32"))


@pytest.mark.parametrize("what,m,length_dtype", PAST, ids=[p[0] for p in PAST])
def test_length_past_the_capacity(gpu, what, m, length_dtype):
    cap = 3 * H.pair_tile(4, 4) + 11
    m = cap + 1 if m is None else m
    a = H.random_bits(cap, "int32", 5).copy()
    v = H.position_values(cap, "uint64")
    for pairs in (True, False):
        k, vv, tk, tv = _dev(a), _dev(v), _poison(a), _poison(v)
        if pairs:
            gpu.sort_pairs_device_devlen_tensor(k, vv, _length(m, length_dtype), tk, tv, check=False)
        else:
            gpu.sort_device_devlen_tensor(k, _length(m, length_dtype), tk, check=False)
        with pytest.raises(gpu.RdstHipError) as e:
            gpu.device_status()
        assert e.value.code == RDST_ERR_DEVICE and "0x20 (" in str(e.value) and "32 = " in str(e.value), str(e.value)
        gpu.device_status()                                          # raised once: clean again
        assert H.same_bits(_host(k, a), a) and H.same_bits(_host(vv, v), v), what
        assert _poisoned_from(tk, a, 0) and _poisoned_from(tv, v, 0), what
        # a valid call right after sorts
        if pairs:
            _check_pairs(gpu, a, v, cap - 7, length_dtype, what + ": the next call")
        else:
            _check_keys(gpu, a, cap - 7, "int32", "uint64", what + ": the next call")


# ---- 5: the length is read in stream order -------------------------------------------------------------------------------

def _stream_order_round(gpu, torch, cap, seed, length_buf=None):
    """keys whose length a device computation enqueued just before the call produces; no .item(), no synchronize between.
    Returns what to check once the stream is idle."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(-(1 << 31), (1 << 31) - 1, (cap,), dtype=torch.int32, device="cuda", generator=g)
    v = torch.arange(cap, dtype=torch.int64, device="cuda")
    orig_a, orig_v = a.clone(), v.clone()
    tk, tv = torch.empty_like(a), torch.empty_like(v)
    mask = torch.rand(cap, device="cuda", generator=g) < (0.3 + 0.4 * (seed % 2))
    count = mask.sum()                                               # a 0-dim int64 tensor on the device: never brought to the host here
    if length_buf is None:
        length_buf = count
    else:
        length_buf.copy_(count)                                      # the same buffer, overwritten on the device
    gpu.sort_pairs_device_devlen_tensor(a, v, length_buf, tk, tv, check=False)
    return a, v, orig_a, orig_v, length_buf, length_buf.clone()          # (the clone: a device copy, enqueued behind the sort)


def _stream_order_check(rec):
    a, v, orig_a, orig_v, _buf, count = rec
    m = int(count.item())
    ha, hv = orig_a.cpu().numpy(), orig_v.cpu().numpy()
    ek, ev = H.expected_pairs(ha[:m], hv[:m])
    ga, gv = a.cpu().numpy(), v.cpu().numpy()
    assert H.same_bits(ga[:m], ek) and H.same_bits(gv[:m], ev)
    assert H.same_bits(ga[m:], ha[m:]) and H.same_bits(gv[m:], hv[m:])
    return m


@pytest.mark.parametrize("own_stream", (False, True), ids=("default stream", "own stream"))
def test_length_is_read_in_stream_order(gpu, own_stream):
    import torch
    cap = 20 * H.pair_tile(4, 8) + 5
    stream = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        first = _stream_order_round(gpu, torch, cap, seed=1)
        # the same length buffer, overwritten on the device with another count, and the same call on fresh data: nothing of
        # the first call's length is kept on the host
        second = _stream_order_round(gpu, torch, cap, seed=2, length_buf=first[4])
        gpu.device_status()
        m1, m2 = _stream_order_check(first), _stream_order_check(second)
        assert abs(m1 - 0.7 * cap) < 0.05 * cap and abs(m2 - 0.3 * cap) < 0.05 * cap


# ---- 6: bounds -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length_dtype", ("int32", "int64"))
def test_every_buffer_stays_inside_its_bands(gpu, length_dtype):
    """keys, values and both tmps at element-aligned offsets that are not 16-byte aligned (the one-key-per-load forms of
    K1 and the copy-back), the length in a banded buffer of its own: read only"""
    lw = np.dtype(length_dtype).itemsize
    # pairs (4, 8)
    cap = 3 * H.pair_tile(4, 8) + 11
    a = _with_equal_keys(H.random_bits(cap, "float32", 9).copy(), 9)
    v = H.position_values(cap, "int64")
    for m in (cap, (cap // 2) | 1, H.pair_tile(4, 8) + 1, 0):
        bk, bv = H.banded(cap, "float32", 4, seed=1, init=a), H.banded(cap, "int64", 8, seed=2, init=v, name="vals")
        btk, btv = H.banded(cap, "float32", 12, seed=3, name="tmp_keys"), H.banded(cap, "int64", 8, seed=4, name="tmp_vals")
        bl = H.banded(1, length_dtype, lw, seed=5, init=np.array([m], dtype=length_dtype), name="length")
        gpu.sort_pairs_device_devlen_tensor(bk["keys"], bv["vals"], bl["length"], btk["tmp_keys"], btv["tmp_vals"])
        ek, ev = D.expected_prefix_sorted(a, m, v)
        assert H.same_bits(H.to_host(bk["keys"], "float32"), ek) and H.same_bits(H.to_host(bv["vals"], "int64"), ev), m
        for b in (bk, bv, btk, btv):
            b.check(f"pairs m = {m}")
        bl.check(f"pairs m = {m}", untouched=("length",))
    # keys only, 2-byte keys at an odd element
    cap = D.small_tile(2) + 3 * D.pass_tile(2, True) + 11
    a = H.random_bits(cap, "int16", 10).copy()
    for m in (cap, (cap // 2) | 1, 1):
        bk, bt = H.banded(cap, "int16", 6, seed=6, init=a), H.banded(cap, "int16", 2, seed=7, name="tmp")
        bl = H.banded(1, length_dtype, lw, seed=8, init=np.array([m], dtype=length_dtype), name="length")
        gpu.sort_device_devlen_tensor(bk["keys"], bl["length"], bt["tmp"])
        assert H.same_bits(H.to_host(bk["keys"], "int16"), D.expected_prefix_sorted(a, m)), m
        bk.check(f"keys m = {m}")
        bt.check(f"keys m = {m}")
        bl.check(f"keys m = {m}", untouched=("length",))
