"""The keys-only sort (rdst_hip_sort_device) through the whole-slice scatter pipeline — K1, K2, K3 and the copy-back — at every
key width: 1-, 2- and 16-byte keys and unsigned 8-byte keys, whose pass shapes are instantiations of their own, with uint32
and float64 beside them.  Levels that K2 skips at both parities of the passes left, copyback_kernel moving data at every
alignment and remainder, crowded digits, single-digit rounds and long equal runs on every tile shape and ranking mode,
chain-split shapes and degenerate orders.  Every case: the result compared bit for bit with the order of the mapped keys
(keys_inputs.expected_sorted), then the device's status word.  tests/test_keys_inputs.py checks, without a device, that each
input is what its name says."""
import numpy as np
import pytest

import helpers as H
import keys_inputs as K

pytestmark = pytest.mark.gpu


def _wide(key):
    return key if H.is_wide(key) else None


def _first_difference(a, b):
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    d = np.flatnonzero((a != b).any(axis=1))
    return f"{d.size} differ, first at {int(d[0])} of {len(a)}" if d.size else "equal"


def _check(gpu, a, key, what, expected=None):
    """sort `a` on the device and compare with the order of the mapped keys"""
    a = np.ascontiguousarray(a)
    exp = K.expected_sorted(a, key) if expected is None else expected
    t = H.to_device(a)
    gpu.sort_device_tensor(t, key=_wide(key))
    got = H.to_host(t, a.dtype).reshape(a.shape)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (key, what, _first_difference(got.view(np.uint8), exp.view(np.uint8)))
    gpu.device_status()


# ---- 1. skipped levels, both pass parities ------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", K.KEY_TYPES)
def test_skipped_levels_at_both_parities(gpu, key):
    """Constant levels are skipped by K2: the first executed level may lie above 0, a pass after a skipped level runs on one
    chain, and an odd number of passes ends in tmp — copyback_kernel<K> moves the keys.  Every length is far below the
    thresholds of the other routes."""
    try:
        for name, _levels, passes, keys in K.constant_level_cases(key):
            _check(gpu, keys, key, (name, f"{passes} passes"))
            assert gpu.last_route() == "lsd", (key, name)
    finally:
        gpu.set_tuning()


# ---- 2. the copy-back moving data -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", K.COPY_BACK_TYPES)
def test_copy_back_forms(gpu, key):
    """An odd number of passes leaves the result in tmp.  copyback_kernel copies 16-byte vectors where both of its pointers
    allow them and single elements elsewhere, and its first block copies what is left behind the last whole vector: keys and
    tmp at element-aligned offsets from a 16-byte boundary, lengths with every remainder of n * sizeof(K) modulo 16 the
    width allows, the bytes around both buffers unchanged."""
    kb = K.key_bytes(key)
    dtype = "uint64" if H.is_wide(key) else key
    remainders = set()
    try:
        for keys in K.copy_back_inputs(key):
            n = len(keys)
            assert (kb - len(K.constant_levels(keys, key))) % 2 == 1       # ends in tmp
            remainders.add(n * kb % 16)
            exp = K.expected_sorted(keys, key)
            for place, ko, to in K.copy_back_placements(key):
                bk = H.banded(keys.shape, dtype, ko, band_bytes=K.COPY_BACK_BAND, seed=1, init=keys)
                bt = H.banded(keys.shape, dtype, to, band_bytes=K.COPY_BACK_BAND, seed=2, name="tmp")
                tk, tt = bk["keys"], bt["tmp"]
                assert (tk.data_ptr() % 16, tt.data_ptr() % 16) == (ko, to)
                gpu.sort_device_tensor(tk, tt, key=_wide(key))
                got = H.to_host(tk, dtype).reshape(keys.shape)
                what = (key, n, place)
                assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (what, _first_difference(got.view(np.uint8), exp.view(np.uint8)))
                bk.check(str(what))
                bt.check(str(what))
                gpu.device_status()
    finally:
        gpu.set_tuning()
    assert remainders == set(range(0, 16, kb))


# ---- 3. heavy digits on every tile shape and ranking mode ------------------------------------------------------------------------

@pytest.mark.parametrize("key", K.KEY_TYPES)
def test_heavy_digits_on_key_tiles(gpu, key):
    """A digit that crowds a wave, rounds of one digit and equal runs longer than a wave's span, at every level named for the
    width.  The shapes with the returning-add ranking (1-, 2-, 4-byte keys and float64) also run with ballots only
    (fast_rank=0) and with every round sent through its fallback (fast_rank=2).  The other bytes are random: a misranked
    round at level 1 or above shows as keys out of order."""
    modes = (True, 0, 2) if key in K.CAN_FAST else (True,)
    try:
        for name, level, a in K.heavy_digit_cases(key):
            exp = K.expected_sorted(a, key)
            for fast in modes:
                gpu.set_tuning(fast_rank=fast)
                _check(gpu, a, key, (len(a), level, name, "fast_rank", fast), expected=exp)
    finally:
        gpu.set_tuning()


# ---- 4. chain-split shapes at 2- and 16-byte tiles ---------------------------------------------------------------------------------

@pytest.mark.parametrize("key", K.CHAIN_SPLIT_TYPES)
def test_chain_split_shapes_at_key_tiles(gpu, key):
    """Previous digits crowded into one group of the chain split or missing from most, a level of two digits, and a slice
    shorter than a tile — with the split on and off."""
    try:
        for name, a in K.chain_split_inputs(key).items():
            exp = K.expected_sorted(a, key)
            for split in (True, False):
                gpu.set_tuning(chain_split=split)
                _check(gpu, a, key, (name, "chain_split", split), expected=exp)
    finally:
        gpu.set_tuning()


# ---- 5. degenerate orders -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", K.DEGENERATE_TYPES)
def test_degenerate_orders(gpu, key):
    """Reverse sorted keys, keys of two values, and keys that differ at one level only (a single pass between skips)."""
    try:
        for name, a in K.degenerate_inputs(key).items():
            _check(gpu, a, key, name)
    finally:
        gpu.set_tuning()
