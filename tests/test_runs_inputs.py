"""The inputs of the run-length tests (tests/runs_inputs.py) checked on the CPU: the constants against the source lines they
quote, the numpy statement of the result against a plain loop, the float keys, the keys that differ in one half only, and that
every shape is what its name says."""
import os
import re

import numpy as np
import pytest

import runs_inputs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(ROOT, "rdst_amd", "csrc", "rdst_runs_layout.h")


def test_constants_are_the_source_s():
    lines = open(LAYOUT).read().splitlines()
    for name, value in (("THREADS", R.THREADS), ("LOOKBACK_WINDOW", R.LOOKBACK_WINDOW)):
        defining = [ln for ln in lines if re.match(rf"constexpr uint32_t {name} = ", ln)]
        assert len(defining) == 1 and defining[0].startswith(f"constexpr uint32_t {name} = {value};"), (name, defining)
    assert "constexpr uint32_t rows(uint32_t elem_bytes) { return elem_bytes >= 8 ? 16 : (elem_bytes == 1 ? 4 : 8); }" in lines
    assert R.ROWS == {b: (16 if b >= 8 else 4 if b == 1 else 8) for b in (1, 2, 4, 8, 16)}
    assert "constexpr uint32_t keys_per_tile(uint32_t elem_bytes) { return THREADS * rows(elem_bytes) * 16 / elem_bytes; }" in lines
    kernel = open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_runs.hip")).read()
    assert f"constexpr uint32_t ERR_RUNS_TRUNCATED = {R.ERR_RUNS_TRUNCATED};" in kernel
    assert f"constexpr uint32_t ERR_LEN_PAST_CAPACITY = {R.ERR_LEN_PAST_CAPACITY};" in kernel
    assert [R.tile(b) for b in (1, 2, 4, 8, 16)] == [16384, 16384, 8192, 8192, 4096]


def test_limits_are_the_constants(hiplib):
    import rdst_amd
    for key, kb in R.KEY_CASES:
        assert rdst_amd.runs_limits(key) == (R.tile(kb), R.LOOKBACK_WINDOW)


@pytest.mark.parametrize("key,kb", R.KEY_CASES)
def test_numpy_statement_against_a_loop(key, kb):
    rng = np.random.default_rng([3, kb])
    for n in (0, 1, 2, 3, 7, 20, 50):
        for longest in (1, 2, 9):
            heads = R.random_runs(n, rng, longest)
            for seed in (0, 5):
                keys = R.keys_from_heads(heads, key, seed=seed)
                assert len(keys) == n and (keys.shape == (n, 2) if R.wide(key) else keys.dtype == np.dtype(key))
                assert np.array_equal(R.heads_of(keys), heads)
                run_keys, starts, count = R.expected(keys)
                loop_starts, loop_count = R.expected_by_loop(keys)
                assert starts.tolist() == loop_starts == np.flatnonzero(heads).tolist() and count == loop_count == len(run_keys)
                assert np.array_equal(R.bits(run_keys), R.bits(keys)[loop_starts])
                for m in (0, n // 2, n):
                    _k, s, c = R.expected(keys, m)
                    assert s.tolist() == [p for p in loop_starts if p < m] and c == len(s)


def test_float_cases_go_by_bits():
    cases = R.float_cases()
    assert len(cases) == 6
    for name, (keys, starts) in cases.items():
        _k, got, count = R.expected(keys)
        assert got.tolist() == starts == R.expected_by_loop(keys)[0] and count == len(starts), name
    zeros = cases["float32: -0.0 and +0.0 are different keys"][0]
    assert np.all(zeros == 0) and np.signbit(zeros).tolist() == [False, False, True, True, False]     # equal as values
    nans = cases["float64: equal NaN bits are one key"][0]
    assert np.all(np.isnan(nans)) and not np.any(nans[1:] == nans[:-1])                                # unequal as values


def test_half_cases_differ_in_one_half_only():
    heads = R.heads_at(50, [1, 2, 9, 30, 49])
    for name, key, half in R.half_cases():
        keys = R.keys_from_heads(heads, key, half=half)
        assert np.array_equal(R.heads_of(keys), heads), name
        b = R.bits(keys)
        if R.wide(key):
            low, high = b[:, 0], b[:, 1]
        else:
            low, high = b & np.uint64(0xFFFFFFFF), b >> np.uint64(32)
        const, varies = (low, high) if half == "high" else (high, low)
        assert len(set(const.tolist())) == 1 and np.array_equal(np.r_[True, varies[1:] != varies[:-1]], heads), name
    assert len(R.half_cases()) == 10


@pytest.mark.parametrize("kb", (1, 2, 4, 8, 16))
def test_shapes_are_what_their_names_say(kb):
    t = R.tile(kb)
    shapes = R.shapes(kb)
    assert [len(shapes[f"random runs, {n} keys"]) for n in R.border_lengths(t)] == [0, 1, 2, t - 1, t, t + 1, 2 * t, 3 * t + 5]
    for name, heads in shapes.items():
        assert len(heads) == 0 or heads[0], name
    for p in (t - 1, t, t + 1):
        assert np.flatnonzero(shapes[f"heads at 0 and {p}"]).tolist() == [0, p]
    assert np.flatnonzero(shapes["heads at T - 1, T and T + 1"]).tolist() == [0, t - 1, t, t + 1]
    assert shapes["all equal"].sum() == 1 and shapes["all distinct"].all()
    six = shapes["one run over tiles 1 .. 3"]
    per_tile = six.reshape(6, t).sum(axis=1)
    assert per_tile[1:4].tolist() == [0, 0, 0] and per_tile[0] > 1 and per_tile[4] > 1 and per_tile[5] > 1
    far = shapes["40 equal tiles, then a distinct one"]
    assert far.reshape(41, t).sum(axis=1).tolist() == [1] + [0] * 39 + [t] and 39 > R.LOOKBACK_WINDOW
    key = {1: "int8", 2: "uint16", 4: "float32", 8: "int64", 16: "u128"}[kb]
    for name, heads in shapes.items():
        assert np.array_equal(R.heads_of(R.keys_from_heads(heads, key)), heads), name
