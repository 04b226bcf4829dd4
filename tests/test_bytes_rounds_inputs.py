"""The inputs of tests/test_gpu_bytes_rounds.py, checked where no device is needed: the constructed order is np.sort's, the
stable expected order is np.lexsort's, and the restated loop of DESIGN.md §2d (helpers.bytes_round_census) reports for every
case exactly the border the case is named for.  The restated constants are compared with the constexpr lines of
rdst_amd/csrc/rdst_bytes.hip, so a change there fails here instead of silently moving a border."""
import os
import re

import numpy as np
import pytest
import torch

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sorted_by_numpy(rows):
    n, N = rows.shape
    return np.sort(np.ascontiguousarray(rows).view(f"V{N}").ravel()).view(np.uint8).reshape(n, N)


def _check_construction(case):
    """the constructed order is THE sorted order, the shuffled rows are a permutation of it, equal keys are equal rows and
    only they, and the stable order of the int64 (run, id) key is np.lexsort's on the key bytes"""
    srt, rows, N = case["sorted"].numpy(), case["rows"].numpy(), case["N"]
    assert np.array_equal(_sorted_by_numpy(rows), srt)
    assert not np.array_equal(rows, srt)
    key, shuffled = case["key"].numpy(), case["key_shuffled"].numpy()
    assert (np.diff(key) >= 0).all()
    assert np.array_equal((srt[1:] == srt[:-1]).all(axis=1), np.diff(key) == 0)
    assert np.array_equal(np.argsort(shuffled, kind="stable"), np.lexsort(rows.T[::-1]))
    return H.bytes_round_census(srt, N)


def test_constants_are_the_sources():
    with open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_bytes.hip")) as f:
        src = f.read()

    def constexpr(name):
        m = re.search(r"constexpr\s+\w+\s+(?:[^;]*?,\s*)?%s\s*=\s*([^,;]+)[,;]" % name, src)
        assert m, name
        expr = m.group(1).strip()
        assert re.fullmatch(r"[\w\s*]+", expr), (name, expr)
        for other in ("SCAN_THREADS", "SCAN_ITEMS"):
            if other in expr:
                expr = expr.replace(other, str(constexpr(other)))
        return eval(expr, {"__builtins__": {}})   # digits, names already replaced, '*'

    assert constexpr("BYTES_SMALL") == H.BYTES_SMALL
    assert constexpr("CMP_WORDS") == H.CMP_WORDS
    assert constexpr("GRID_CAP") == H.BYTES_GRID_CAP
    assert constexpr("CMP_WAVES") == H.CMP_WAVES
    assert constexpr("SCAN_TILE") == H.BYTES_SCAN_TILE
    assert "if (blocks > (1u << 20)) blocks = 1u << 20;" in src and H.SHORT_RUNS_BLOCKS == 1 << 20
    assert "return len > BYTES_SMALL || (uint64_t)len * words > CMP_WORDS;" in src
    assert H.GRID_ROWS == 1 << 20 and H.SHORT_RUNS_PER_TRIP == 1 << 22


def test_long_round_bits():
    assert {runs: H.long_round_bits(runs) for runs in H.LAYOUT_LONG_RUNS} == H.LAYOUT_LONG_RUNS
    assert H.long_round_bits(0) == (0, 8) and H.long_round_bits(4) == (2, 7) and H.long_round_bits(5) == (3, 7)


@pytest.mark.parametrize("N", H.RANK_WIDTHS)
def test_ranking_cases(N):
    """39 runs of 2 ... 256 rows, all short, every length with a kind that word 0 does not decide"""
    runs, k = H.ranking_runs(N)
    case = H.bytes_round_case(torch, runs, N, k, seed=N)
    census = _check_construction(case)
    assert len(census) == 1
    c = census[0]
    assert (c["runs"], c["long_runs"], c["short_max"], c["short_trips"]) == (39, 0, 256, 1)
    assert c["words"] == {20: 3, 41: 9, 68: 15}[N] and c["tied"] == 3 * sum(H.RANK_LENGTHS)
    if N == 68:
        assert c["short_max"] * c["words"] == H.CMP_WORDS      # 256 rows x 15 words = 3 840, short
    tied = [r for r in runs if r[0] > 1]
    by_length = {}
    for length, kind in tied:
        by_length.setdefault(length, set()).add(kind.split("+")[0])
    assert sorted(by_length) == list(H.RANK_LENGTHS)
    assert all(kinds & {"later", "last", "straddle"} for kinds in by_length.values())       # decided past word 0
    assert {kind.split("+")[0] for _l, kind in tied} == set(H.ROUND_KINDS)
    assert any(kind.endswith("+dups") and length >= 65 for length, kind in tied)
    assert any(not kind.endswith("+dups") and kind != "dup" and length >= 65 for length, kind in tied)
    # where the deciding bytes lie, read from the rows: a run's first differing column
    srt, key = case["sorted"].numpy(), case["key"].numpy()
    run_of = key >> H.ROUND_ID_BITS
    seen = set()
    start = 0
    for length, kind in runs:
        if length > 1 and kind != "dup":
            block = srt[start:start + length]
            cols = np.flatnonzero((block != block[0]).any(axis=0))
            assert len(set(run_of[start:start + length])) == 1 and cols[0] >= 8
            first, base = cols[0] - 8, kind.split("+")[0]
            if base == "word0":
                assert first < 4
            elif base == "later":
                assert first >= 4 and first % 4 <= 1
            elif base == "last":
                assert first == N - 9 and {0, 1} <= set(block[:, -1].tolist())
            else:
                assert first == (k if length <= 16 else k - 1)      # up to 16 rows share the high byte
            seen.add((base, int(first) // 4))
        start += length
    assert ("last", c["words"] - 1) in seen and any(b == "later" and w >= 1 for b, w in seen)
    if N == 41:
        assert (N - 8) % 4 == 1                                      # the last word: one key byte, three of padding


def test_staging_budget_classifications():
    expect = {(68, 256): False, (68, 257): True, (72, 240): False, (72, 241): True, (1000, 15): False, (1000, 16): True,
              (3848, 4): False, (3848, 5): True, (3849, 3): False, (3849, 4): True, (4096, 3): False, (4096, 4): True}
    for (N, length), is_long in expect.items():
        assert H.run_is_long(length, (N - 8 + 3) // 4) == is_long, (N, length)
    assert (68 - 8) // 4 * 256 == 3840 and (72 - 8) // 4 * 240 == 3840 and (3848 - 8) // 4 * 4 == 3840
    assert {(N, s) for N, s, _l in H.BUDGET_PAIRS} | {(N, l) for N, _s, l in H.BUDGET_PAIRS} == set(expect)


@pytest.mark.parametrize("N,short,long", H.BUDGET_PAIRS)
def test_staging_budget_cases(N, short, long):
    """one run stays with the comparison kernel, its neighbour one row longer goes to the pair sort, where it stays tied
    until its last byte"""
    runs, k = H.budget_runs(N, short, long)
    case = H.bytes_round_case(torch, runs, N, k, seed=N)
    census = _check_construction(case)
    c = census[0]
    assert (c["runs"], c["long_runs"], c["long_rows"], c["short_max"], c["b"], c["k"]) == (2, 1, long, short, 0, 8)
    assert short * c["words"] <= H.CMP_WORDS
    assert long > H.BYTES_SMALL or long * c["words"] > H.CMP_WORDS
    assert len(census) >= 2 and all(r["tied"] == long and r["runs"] == 1 for r in census[1:])     # one run, whole, to the end
    last = census[-1]
    assert last["depth"] + 8 >= N or last["long_runs"] == 0         # the last byte is read by the last round


@pytest.mark.parametrize("N", (17, 29))
@pytest.mark.parametrize("long_runs", (1, 2, 3, 256, 257))
def test_layout_cases(long_runs, N):
    """exactly `long_runs` long runs in the first long round: b and k at their borders; rows that stay tied behind it and
    separate one and two rounds later"""
    runs, k = H.layout_runs(long_runs)
    case = H.bytes_round_case(torch, runs, N, k, seed=long_runs * 100 + N)
    census = _check_construction(case)
    c = census[0]
    assert (c["long_runs"], c["b"], c["k"]) == (long_runs, *H.LAYOUT_LONG_RUNS[long_runs]) and c["k"] == k
    assert c["long_rows"] == 257 * long_runs and c["runs"] > long_runs          # short runs in the same round
    assert c == H.bytes_first_round([r[0] for r in runs], N)
    assert len(census) >= 2
    second = census[1]
    assert second["depth"] == 8 + k and second["m"] == c["long_rows"]
    if long_runs >= 2:
        # the straddled pairs: tied in sixteens behind byte 8 + k - 1, apart one byte later (short runs of the second round)
        assert second["runs"] > second["long_runs"] >= 1 and second["short_max"] >= 16
    else:
        assert second["runs"] == 16 and second["long_runs"] == 0 and second["short_max"] == 16   # 16 x 16 rows and one alone
    if N == 29 and long_runs >= 2:
        assert len(census) >= 3 and census[2]["depth"] == 8 + k + second["k"] and census[2]["tied"] > 0   # a third pair sort
    if N == 17 and long_runs >= 2:
        assert second["depth"] + second["k"] >= N                  # the second long round reads to N or past it (zeros)
    srt = case["sorted"].numpy()
    assert len(np.unique(srt[:, 8 + k - 1])) > 16 and len(np.unique(srt[:, 8 + k])) > 16      # both bytes at the border busy


@pytest.mark.parametrize("long_runs", (65_536, 65_537))
def test_layout_cases_on_the_device_scaled_down(long_runs):
    """the two largest layout cases are built on the device; here: their first round from the run lengths (b = 16 / 17,
    k = 6 / 5, second trips of the keys, long-rows and slot kernels), and the same tensors at 515 runs against numpy"""
    N = 17
    lengths, kinds, dups = H.layout_tensors(torch, long_runs, "cpu")
    first = H.bytes_first_round(lengths.numpy(), N)
    b, k = H.LAYOUT_LONG_RUNS[long_runs]
    assert (first["long_runs"], first["b"], first["k"]) == (long_runs, b, k)
    assert first["long_rows"] == 257 * long_runs and first["long_trips"] == 17 and first["scan_trips"] == 17
    assert 8 + k < N < 8 + 2 * k                     # the second long round ends past N: its last bytes are the zero padding
    lengths, kinds, dups = H.layout_tensors(torch, 515, "cpu")
    case = H.bytes_round_rows(torch, lengths, kinds, N, k, seed=long_runs, dups=dups)
    census = _check_construction(case)
    assert census[0] == H.bytes_first_round(lengths.numpy(), N) and census[0]["long_runs"] == 515
    assert len(census) >= 2 and census[1]["runs"] > census[1]["long_runs"] >= 1
    assert len(np.unique(case["sorted"].numpy()[:, 8 + k - 1])) > 16


def test_short_run_grid_stride_case_scaled_down():
    """second trip of short_runs_kernel: more than 4 x 2^20 short runs at full size (from the lengths alone); the same
    tensors at a thousandth of the size against numpy"""
    N = 17
    lengths, kinds, dups = H.stride_tensors(torch, "cpu")
    ln = lengths.numpy()
    first = H.bytes_first_round(ln, N)
    assert first["runs"] == H.STRIDE_PAIRS + H.STRIDE_MID > H.SHORT_RUNS_PER_TRIP and first["long_runs"] == 0
    assert first["short_trips"] == 2
    mid = ln[ln > 2]
    assert len(mid) == H.STRIDE_MID and mid.min() == 65 and mid.max() == 256 and (ln[ln <= 2] == 2).all()
    where = np.flatnonzero(ln > 2)
    assert (where < H.SHORT_RUNS_PER_TRIP).any() and (where >= H.SHORT_RUNS_PER_TRIP).any()     # runs of both trips
    assert first["m"] < 9_000_000
    lengths, kinds, dups = H.stride_tensors(torch, "cpu", pairs=4_200, mid=20)
    case = H.bytes_round_rows(torch, lengths, kinds, N, 8, seed=4, dups=dups)
    census = _check_construction(case)
    assert len(census) == 1 and census[0]["runs"] == 4_220 and census[0]["short_max"] > 64
    assert census[0] == H.bytes_first_round(lengths.numpy(), N)


def test_records_form():
    runs, k = H.ranking_runs(20)
    case = H.bytes_round_case(torch, runs, 20, k, seed=20)
    rec = H.bytes_round_records(case, seed=1)
    raw, dt = rec["raw"], rec["dtype"]
    assert dt.itemsize == 28 and dt.fields["k"][1] == 1 and raw.shape == (case["n"], 28)
    keys = raw[:, 1:21]
    assert np.array_equal(rec["by_key"], raw[np.lexsort(keys.T[::-1])])
    inv = (~raw[:, :1]).copy()                                      # descending: the complemented byte, ascending
    assert np.array_equal(rec["by_key_tag_desc"], raw[np.lexsort(np.concatenate([keys, inv], axis=1).T[::-1])])
    assert not np.array_equal(rec["by_key"], rec["by_key_tag_desc"])
    seq = np.ascontiguousarray(rec["by_key"][:, 24:28]).view("<u4").ravel()
    assert np.array_equal(np.sort(seq), np.arange(case["n"]))
    # equal keys: seq ascending inside every run of equal keys, and such runs of 65 rows and more exist
    k_sorted = rec["by_key"][:, 1:21]
    eq = (k_sorted[1:] == k_sorted[:-1]).all(axis=1)
    assert eq.sum() > 1000 and (np.diff(seq.astype(np.int64))[eq] > 0).all()
    assert len(np.unique(raw[:, 21:24], axis=0)) > case["n"] // 2   # the junk behind the key is random


def test_census_on_a_hand_made_input():
    """rows small enough to follow by eye: 300 rows sharing 17 bytes, then four values of byte 17, then distinct tails"""
    N = 24
    rows = np.zeros((300 + 3, N), dtype=np.uint8)
    rows[:300, 17] = np.repeat(np.arange(4), 75)
    rows[:300, 23] = np.tile(np.arange(75), 4)
    rows[300:, 0] = (1, 2, 3)
    census = H.bytes_round_census(rows, N)
    assert [(c["depth"], c["words"], c["tied"], c["runs"], c["long_rows"], c["long_runs"]) for c in census] == \
        [(8, 4, 300, 1, 300, 1), (16, 2, 300, 1, 300, 1)]           # depth 24 = N: no third round
    rows[:300, 15] = np.repeat(np.arange(2), 150)                 # decided inside the first long round: two runs behind it
    census = H.bytes_round_census(rows, N)
    assert [(c["depth"], c["tied"], c["runs"], c["long_runs"], c["short_max"]) for c in census] == [(8, 300, 1, 1, 0), (16, 300, 2, 0, 150)]
