"""The guard-band detector of tests/helpers.py (Bands / banded) on CPU torch tensors and numpy arrays: it must flag one
changed byte at either end of every band, leave writes inside a view alone, and name the changed bytes relative to the
view — otherwise tests/test_gpu_bounds.py could pass without looking."""
import numpy as np
import pytest

from helpers import DTYPES, SMALL_DTYPES, Bands, banded, mapped_key, poison_pattern, random_bits, without_poison

BAND = 1024


def _devices():
    out = [None]
    try:
        import torch  # noqa: F401
        out.append("cpu")
    except ImportError:
        pass
    return out


def _poke(b, i):
    """flip every bit of byte `i` of the allocation"""
    if b.device is None:
        b.raw[i] ^= 0xFF
    else:
        b.raw[i] = int(b.raw[i]) ^ 0xFF


def _fill_view(v, value):
    v[...] = value


@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("offset", (0, 4, 12, 0x100))
def test_one_byte_at_either_end_of_each_band_is_flagged(device, offset):
    n = 100
    b = banded(n, "uint32", offset, BAND, seed=1, device=device, init=np.arange(n, dtype=np.uint32))
    _n, s, e, _shape, _dt = b.span("keys")
    assert s == BAND + offset and e == s + 4 * n
    b.check("fresh")
    total = b.image.size
    cases = {0: f"bytes [-{s}, -{s - 1}) before keys[0]", s - 1: "bytes [-1, -0) before keys[0]",
             e: "bytes [+0, +1) after keys[len)", total - 1: f"bytes [+{total - 1 - e}, +{total - e}) after keys[len)"}
    for i, want in cases.items():
        _poke(b, i)
        with pytest.raises(AssertionError) as err:
            b.check("poked")
        assert want in str(err.value), (i, str(err.value))
        _poke(b, i)
        b.check("restored")
    assert total - e >= BAND                          # never flush with the end of the allocation


@pytest.mark.parametrize("device", _devices())
def test_writes_inside_the_view_are_not_flagged(device):
    b = banded(257, "float64", 8, BAND, seed=2, device=device)
    _fill_view(b["keys"], 3.0)
    b.check("inside")
    with pytest.raises(AssertionError, match=r"bytes \[0, 2056\) of keys, which must stay untouched"):
        b.check("inside, read-only", untouched=("keys",))


@pytest.mark.parametrize("device", _devices())
def test_reported_offsets_span_first_to_last_changed_byte(device):
    b = banded(64, "uint64", 8, BAND, seed=3, device=device)
    _n, s, e, _shape, _dt = b.span("keys")
    for i in (e + 16, e + 31):
        _poke(b, i)
    _poke(b, s - 8)
    with pytest.raises(AssertionError) as err:
        b.check("two bands")
    msg = str(err.value)
    assert "bytes [+16, +32) after keys[len) changed (2 differ)" in msg
    assert "bytes [-8, -7) before keys[0] changed (1 differ)" in msg


@pytest.mark.parametrize("device", _devices())
def test_views_share_one_allocation_and_the_gaps_are_bands(device):
    a = random_bits(50, "int32", 4)
    b = Bands([("first", a, 4), ("second", ((30,), "int64"), 0x104)], BAND, seed=5, device=device)   # (8-aligned)
    _n, s1, e1, _shape, _dt = b.span("first")
    _n, s2, e2, _shape, _dt = b.span("second")
    assert s1 == BAND + 4 and s2 == e1 + 0x104 and b.image.size - e2 >= BAND
    got = b["first"] if device is None else b["first"].numpy()
    assert np.array_equal(got, a)
    _poke(b, e1 + 0xFF)
    with pytest.raises(AssertionError, match=r"bytes \[\+255, \+256\) after first\[len\)"):
        b.check("gap")


@pytest.mark.parametrize("device", _devices())
def test_extended_view_reaches_into_the_band_and_is_still_checked(device):
    b = banded(10, "uint32", 4, BAND, seed=6, device=device)
    t = b.extended("keys", 64)
    assert t.shape[0] == 26
    t[10] = 0 if int(t[10]) else 1
    with pytest.raises(AssertionError, match=r"bytes \[\+0, \+\d\) after keys\[len\)"):
        b.check("extended")


def test_host_views_are_aligned_like_device_allocations():
    for off in (0, 1, 3, 4, 8, 0x100):
        b = banded(33, "uint8", off, BAND, seed=7, device=None)
        assert b["keys"].ctypes.data % 256 == off % 256
        assert b["keys"].flags.c_contiguous and b["keys"].flags.writeable


@pytest.mark.parametrize("dtype", DTYPES + SMALL_DTYPES)
def test_poison_is_the_smallest_mapped_key_and_is_removed_from_inputs(dtype):
    nb = np.dtype(dtype).itemsize
    p = poison_pattern(dtype)
    assert p.size == nb
    assert int(mapped_key(p.view(dtype))[0]) == 0
    a = random_bits(5000, dtype, 8).copy()
    a[::7] = p.view(dtype)[0]
    c = without_poison(a)
    u, pu = c.view(f"u{nb}"), p.view(f"u{nb}")[0]
    assert not (u == pu).any()
    keep = a.view(f"u{nb}") != pu
    assert keep.sum() < a.size and (u[keep] == a.view(f"u{nb}")[keep]).all()   # the other keys stay


def test_poison_fill_repeats_the_key_on_the_element_grid():
    b = banded(16, "float32", 12, BAND, fill=poison_pattern("float32"), device=None)
    assert (b.image[:b.span("keys")[1]] == 0xFF).all()
    b = banded(16, "int16", 6, BAND, fill=poison_pattern("int16"), device=None)
    s = b.span("keys")[1]
    assert (b.image[:s].view("<u2") == 0x8000).all() and s % 2 == 0
    rows = np.zeros((5, 3), dtype=np.uint8)
    assert (without_poison(rows, "bytes")[:, -1] == 1).all()
    limbs = np.zeros((4, 2), dtype=np.uint64)
    limbs[1, 1] = 5
    w = without_poison(limbs, "u128")
    assert w[0, 0] == 1 and w[1, 0] == 0 and w[1, 1] == 5
