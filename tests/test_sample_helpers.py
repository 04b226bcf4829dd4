"""The builders of tests/test_gpu_sample.py held to their names (CPU): each produces the sample verdict it promises AND the
ground truth it promises, so that a later edit cannot quietly turn an adversarial input into a harmless one."""
import numpy as np
import pytest

import helpers as H

N0 = (1 << 26) + 12_345
LENGTHS = (N0, 3 * (1 << 26) + 16_897, 100_000_003, (1 << 29) + 12_345, 68_721_573, 68_721_574, 3_000_001)
WIDTH = {"uint32": 32, "int32": 32, "float32": 32, "uint64": 64, "int64": 64, "float64": 64}
T = H.route_tuning(1, 1)
ZERO = dict.fromkeys(H.SAMPLE_WORDS, 0)


def _gen(seed=1):
    import torch
    return torch.Generator().manual_seed(seed)


def _verdict(m, name, n=N0, t=T):
    import torch
    return H.sample_verdict(H.unmapped_bits(torch, m, name).numpy().view(name), t, n=n)


def _unsigned(m, name):
    """the mapped keys a tensor of mapped bits stands for, through the key type and back"""
    import torch
    return H.mapped_key(H.unmapped_bits(torch, m, name).numpy().view(name))


@pytest.mark.parametrize("name", H.DTYPES)
def test_unmapped_inverts_mapped_key(name):
    import torch
    a = H.random_bits(100_000, name, seed=3)
    assert H.same_bits(H.unmapped(H.mapped_key(a), name), a)
    m = torch.from_numpy(H.mapped_key(a).view(f"i{a.dtype.itemsize}").copy())
    assert np.array_equal(H.unmapped_bits(torch, m, name).numpy().view(f"u{a.dtype.itemsize}"), H.uint_view(a))


def test_sample_positions_stay_inside():
    for n in LENGTHS:
        p = H.sample_positions(n)
        assert len(p) == 8192 and p[0] == 0 and p[-1] < n and (np.diff(p) == n // 8192).all()
        if n >= H.PRESAMPLE_MIN_LEN:
            assert n % 8192 != 0
        for kb in (4, 8):
            if n >= H.PRESAMPLE_MIN_LEN:
                H.stray_positions(n, kb)                       # (asserts that none of them is sampled)
            spots = H.swap_spots(n, kb)
            g = H.pass_a_geometry(kb)
            assert {0, 63, g["span"] - 1, g["tile"] - 1, g["tile"], n - 2} <= set(spots) and len(spots) >= 20


def test_pass_a_geometry():
    assert H.pass_a_geometry(4) == {"kpt": 22, "span": 1408, "tile": 16896}
    assert H.pass_a_geometry(8) == {"kpt": 11, "span": 704, "tile": 8448}


def test_the_issue_s_five_inputs():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 1 << 32, size=N0, dtype=np.uint32)
    assert H.sample_verdict(a, T) == ZERO
    low = a[H.sample_positions(N0)] & 0xFFFF
    assert 400 < len(low) - len(np.unique(low)) < 600          # ~500 repeated low halves on uniform keys
    assert H.sample_verdict(a >> 2, T) == dict(ZERO, win_shift=2)
    c = np.full(N0, 0x47474747, dtype=np.uint32)
    c[-1] = 5
    assert H.sample_verdict(c, T) == dict(win_shift=8, win_top=0x47, gross_skew=1, top_skew=1, low_dups=1, predict_lsd=0)
    c = np.full(N0, 0x4747474747474747, dtype=np.uint64)
    c[-1] = 5
    assert H.sample_verdict(c, T) == dict(win_shift=8, win_top=0x47, gross_skew=1, top_skew=1, low_dups=0, predict_lsd=1)
    d = a.copy()
    p = H.sample_positions(N0)
    d[p] = (d[p] & 0xFFFFFF) | (0x47 << 24)
    assert H.sample_verdict(d, T) == dict(ZERO, win_shift=8, win_top=0x47)
    # no sample: a short slice, the LSD-only setting, mode 5, and the shipped threshold of 4-byte keys
    assert H.sample_verdict(c[:8192], T, n=N0 - 20_000) == ZERO
    for t in (H.route_tuning(0, 1), H.route_tuning(5, 1)):
        assert H.sample_verdict(c, t) == ZERO
    assert H.sample_verdict(d, H.route_tuning(1, 0)) == ZERO and H.routes_tried(N0, 8, H.route_tuning(1, 0)) == (True, False)


@pytest.mark.parametrize("name", list(WIDTH))
def test_window_keys_share_exactly_d_bits(name):
    import torch
    w, n = WIDTH[name], 200_000
    for d in (0, 1, 4, 8, 9, 12, 16):
        for kind in ("zeros", "ones", "mixed"):
            pat = H.window_pattern(kind, d)
            m = H.window_keys(torch, n, w, d, pat, _gen(d), "cpu")
            u = _unsigned(m, name).astype(np.uint64)
            assert d == 0 or ((u >> np.uint64(w - d)) == pat).all()
            s = u[H.sample_positions(n)]
            if d < 16:
                assert len(np.unique((s >> np.uint64(w - d - 1)) & np.uint64(1))) == 2   # the next bit: both values, in the sample
            v = _verdict(m[H.sample_index(torch, n, "cpu")], name)
            assert v["win_shift"] == min(d, 8) and v["win_top"] == (pat >> max(0, d - 8) if d else 0)


def test_a_stray_is_one_key_outside_the_window():
    import torch
    n, w, d = 300_000, 32, 4
    pat = H.window_pattern("mixed", d)
    for flip in (1, 8):
        m = H.window_keys(torch, n, w, d, pat, _gen(5), "cpu")
        pos = H.not_sampled(n, [n - 1])[0]
        m[pos:pos + 1] = H.set_top(m[pos:pos + 1], w, d, pat ^ flip)
        out = H.top_bits(m, w, d) != pat
        assert int(out.sum()) == 1 and bool(out[pos]) and int(H.top_bits(m, w, d)[pos]) == pat ^ flip
        assert _verdict(m[H.sample_index(torch, n, "cpu")], "uint32")["win_shift"] == d


@pytest.mark.parametrize("name", ["uint32", "float32", "int64"])
def test_threshold_samples(name):
    import torch
    w = WIDTH[name]
    lim = 12 + 4 * H.LOCAL_TILE[w // 8] * 8192 // N0
    assert lim == (20 if w == 32 else 19)
    assert _verdict(H.spread_sample(torch, w, _gen(), "cpu"), name) == ZERO
    for hits in (lim - 1, lim):
        m = H.gross_sample(torch, w, hits, _gen(), "cpu")
        counts = np.bincount((_unsigned(m, name).astype(np.uint64) >> np.uint64(w - 16)).astype(np.int64), minlength=65536)
        assert counts.max() == hits and counts[0xF008] == hits and (np.delete(counts, 0xF008) <= 1).all()
        assert _verdict(m, name) == dict(ZERO, gross_skew=int(hits >= lim))
    for hits in (63, 64):
        m = H.top_sample(torch, w, hits, _gen(), "cpu")
        u = _unsigned(m, name).astype(np.uint64)
        assert np.bincount((u >> np.uint64(w - 8)).astype(np.int64), minlength=256).max() == hits
        assert np.bincount((u >> np.uint64(w - 16)).astype(np.int64)).max() == 1
        assert _verdict(m, name) == dict(ZERO, top_skew=int(hits >= 64))


def test_low_half_and_prediction_samples():
    import torch
    for dups in (4999, 5000):
        m = H.dups_sample(torch, dups, _gen(), "cpu")
        low = _unsigned(m, "uint32") & 0xFFFF
        assert 8192 - len(np.unique(low)) == dups and np.bincount(low).max() < 256
        assert _verdict(m, "uint32") == dict(ZERO, low_dups=int(dups >= 5000))
    n29 = (1 << 29) + 12_345
    for nbytes in (24, 25):
        m = H.bytes_sample(torch, 32, nbytes, 320, _gen(), "cpu")
        hits = np.bincount(_unsigned(m, "uint32") >> 24, minlength=256)
        assert (hits == 320).sum() == nbytes and n29 * 320 // (8192 * 256) >= 81920 > n29 * 319 // (8192 * 256)
        assert _verdict(m, "uint32", n29) == dict(ZERO, top_skew=1, predict_lsd=int(nbytes >= 25))
        assert _verdict(m, "uint32", n29, H.route_tuning(14, 1)) == dict(ZERO, top_skew=1)
    for hits in (2559, 2560):                                   # without the giant kernels one giant-sized byte predicts
        m = H.bytes_sample(torch, 32, 1, hits, _gen(), "cpu")
        assert _verdict(m, "uint32", N0, H.route_tuning(11, 1)) == dict(ZERO, top_skew=1, predict_lsd=int(hits >= 2560))
        assert _verdict(m, "uint32") == dict(ZERO, top_skew=1)
    for hits in (1023, 1024):
        m = H.bytes_sample(torch, 64, 1, hits, _gen(), "cpu")
        assert _verdict(m, "uint64") == dict(ZERO, top_skew=1, predict_lsd=int(hits >= 1024))
    m = H.bytes_sample(torch, 64, 1, 1000, _gen(), "cpu")
    assert 68_721_573 * 1000 // (8192 * 256) == 2 * H.LOCAL_TILE[8] and 68_721_574 * 1000 // (8192 * 256) == 2 * H.LOCAL_TILE[8] + 1
    assert _verdict(m, "uint64", 68_721_573)["predict_lsd"] == 0 and _verdict(m, "uint64", 68_721_574)["predict_lsd"] == 1
    # the population that holds what the sample shows: the same share of the keys on the same top bytes
    pop = H.bytes_population(torch, H.rand_mapped(torch, 8192 * 40, 32, _gen(), "cpu"), 32, 25, 320)
    share = np.bincount(_unsigned(pop, "uint32") >> 24, minlength=256) / pop.numel()
    assert all(abs(share[16 + 8 * j] - 320 / 8192) < 0.002 for j in range(25)) and share[8] < 0.002


@pytest.mark.parametrize("w", [32, 64])
def test_increasing_keys_increase(w):
    import torch
    n = 300_000
    for kw in ({}, {"below_bits": w - 2}, {"dense_from": 0x2000_0000}):
        u = _unsigned(H.increasing_keys(torch, n, w, _gen(), "cpu", **kw), f"uint{w}")
        assert (u[1:] > u[:-1]).all()
        if "below_bits" in kw:
            assert int(u[-1]) < 1 << (w - 2) and int(u[-1]) > 1 << (w - 3)
        if not kw:
            assert int(u[-1]) >> (w - 1) == 1                  # the whole range


def test_route_rules_on_the_plain_cases():
    clean = dict(ZERO)
    t = H.route_tuning(1, 1)
    assert H.predicted_route(clean, N0, 4, t, True, 0, 1100) == "atomic"
    assert H.predicted_route(clean, N0, 4, t, None, 0, 1100) is None
    assert H.predicted_route(clean, N0, 4, t, False, 1, N0) == "hybrid"              # a giant bucket the sample never saw
    assert H.predicted_route(clean, N0, 8, t, False, 1, N0) == "lsd"                  # 8-byte keys: over the tile
    assert H.predicted_route(clean, N0, 4, H.route_tuning(10, 1), False, 0, 1100) == "lsd"
    assert H.predicted_route(clean, N0, 4, H.route_tuning(11, 1), False, 1, N0) == "lsd"
    assert H.predicted_route(dict(ZERO, predict_lsd=1), N0, 8, t, True, 0, 1100) == "lsd"
    assert H.predicted_route(dict(ZERO, gross_skew=1), N0, 8, t, True, 0, 1100) == "lsd"
    assert H.predicted_route(dict(ZERO, gross_skew=1), N0, 4, t, True, 0, 1100) == "hybrid"
    assert H.predicted_route(dict(ZERO, top_skew=1), N0, 8, t, True, 0, 1100) == "hybrid"
    assert H.predicted_route(clean, 3 * (1 << 26) + 16_897, 4, H.route_tuning(1, 0), False, 0, 4000) == "lsd"
