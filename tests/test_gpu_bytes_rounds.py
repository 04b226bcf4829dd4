"""The refinement rounds of the wide [u8; N] route (rdst_amd/csrc/rdst_bytes.hip) at their own borders:
the comparison kernel's ranking on runs of 2 ... 256 rows decided in every word, the staging budget on both sides, the
long-run key layout where b and k step, the second trips of every grid-stride loop, stability of records whose keys stay
tied through the rounds, and the N <= 16 widened route past its grid cap.

Every input is constructed (helpers.bytes_round_rows): the sorted rows are known without sorting, and the stable order of
records is the stable order of an int64 (run, id) key.  tests/test_bytes_rounds_inputs.py shows on the CPU, case by case,
that each input reaches the border it is named for (helpers.bytes_round_census restates the loop)."""
import functools

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

UNSIGNED, BYTES_BE = 0, 3
SPLIT_AT = 11        # the key as two adjacent byte-string fields: the second starts inside the first refinement word


def F(offset, nbytes, kind, descending=False):
    from rdst_amd import KeyField
    return KeyField(offset, nbytes, kind, descending)


def _sorted_by_numpy(rows):
    n, N = rows.shape
    return np.sort(np.ascontiguousarray(rows).view(f"V{N}").ravel()).view(np.uint8).reshape(n, N)


@functools.lru_cache(maxsize=None)
def _case(group, *args):
    """the host cases, built once and shared by the rows test and the records test of the same input (never modified)"""
    import torch
    if group == "ranking":
        (N,) = args
        runs, k = H.ranking_runs(N)
        seed = N
    elif group == "budget":
        N, short, long = args
        runs, k = H.budget_runs(N, short, long)
        seed = N
    else:
        long_runs, N = args
        runs, k = H.layout_runs(long_runs)
        seed = long_runs * 100 + N
    case = H.bytes_round_case(torch, runs, N, k, seed=seed)
    case["first_round"] = H.bytes_first_round([r[0] for r in runs], N)
    return case


def _check_rows(gpu, case):
    """device entry and host entry, element for element against the constructed answer and against np.sort of V<N>"""
    assert case["n"] <= 300_000
    want = case["sorted"].numpy()
    t = case["rows"].cuda()
    gpu.sort_bytes_device_tensor(t)
    got = t.cpu().numpy()
    assert np.array_equal(got, want), "device entry"
    host = case["rows"].numpy().copy()
    gpu.sort_host_array(host, key="bytes")
    assert np.array_equal(host, want), "host entry"
    assert np.array_equal(_sorted_by_numpy(case["rows"].numpy()), want)
    gpu.device_status()


def _check_on_device(gpu, case):
    import torch
    t = case["rows"].clone()
    gpu.sort_bytes_device_tensor(t)
    assert torch.equal(t, case["sorted"])
    gpu.device_status()


def _check_records(gpu, case, seed):
    """the same rows as keys of records: the single-field host entry (stride R, key at offset 1), the described-key device
    entry with one field, and with the key split in two fields plus a descending tag (packed rows of stride L); whole
    records compared with the stable order of the int64 key"""
    import torch
    N = case["N"]
    rec = H.bytes_round_records(case, seed)
    raw, dt = rec["raw"], rec["dtype"]
    arr = raw.copy().view(dt).reshape(-1)
    gpu.sort_host_records(arr, "k")
    assert np.array_equal(arr.view(np.uint8).reshape(raw.shape), rec["by_key"]), "host entry, single field"
    t = torch.from_numpy(raw).cuda()
    gpu.sort_records_device_tensor(t, [F(1, N, BYTES_BE)])
    assert np.array_equal(t.cpu().numpy(), rec["by_key"]), "device entry, one field"
    split = [F(1, SPLIT_AT, BYTES_BE), F(1 + SPLIT_AT, N - SPLIT_AT, BYTES_BE)]
    t = torch.from_numpy(raw).cuda()
    if N + 1 <= 4096:                                   # (a described key holds at most 4096 bytes)
        gpu.sort_records_device_tensor(t, split + [F(0, 1, UNSIGNED, True)])
        assert np.array_equal(t.cpu().numpy(), rec["by_key_tag_desc"]), "device entry, split key and a descending tag"
    else:
        gpu.sort_records_device_tensor(t, split)
        assert np.array_equal(t.cpu().numpy(), rec["by_key"]), "device entry, split key"
    gpu.device_status()


LAYOUT_SMALL = [(long_runs, N) for long_runs in (1, 2, 3, 256, 257) for N in (17, 29)]


# ---- a. ranking in the comparison kernel -----------------------------------------------------------------------------------

@pytest.mark.parametrize("N", H.RANK_WIDTHS)
def test_ranking_of_short_runs(gpu, N):
    """39 runs of 2, 3, 63 ... 256 rows among 5 000 unrelated rows: decided in word 0, in a later word only, in the last
    byte (N = 41: of a padded word), across the border of words 0 and 1, not at all; all distinct and with a third of the
    rows repeated.  N = 68: 256 rows x 15 words, the whole staging budget."""
    case = _case("ranking", N)
    assert case["first_round"]["long_runs"] == 0 and case["first_round"]["short_max"] == 256
    _check_rows(gpu, case)


# ---- b. staging budget -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,short,long", H.BUDGET_PAIRS)
def test_staging_budget_both_sides(gpu, N, short, long):
    """two runs of distinct rows decided in the last byte: `short` rows x words <= 3 840 (comparison kernel), `long` one
    row more (pair-sort rounds until the run fits, or to the last byte)"""
    case = _case("budget", N, short, long)
    first = case["first_round"]
    assert (first["short_max"], first["long_rows"], first["long_runs"]) == (short, long, 1)
    _check_rows(gpu, case)


# ---- c. long-run key layout --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("long_runs,N", LAYOUT_SMALL)
def test_long_run_key_layout(gpu, long_runs, N):
    """exactly 1, 2, 3, 256, 257 long runs: (b, k) = (0, 8), (1, 7), (2, 7), (8, 7), (9, 6); deciding bytes on both sides of
    the first round's last byte, rows that part one and two rounds later, duplicates that never part"""
    case = _case("layout", long_runs, N)
    first = case["first_round"]
    assert (first["long_runs"], first["b"], first["k"]) == (long_runs, *H.LAYOUT_LONG_RUNS[long_runs])
    _check_rows(gpu, case)


@pytest.mark.parametrize("long_runs", (65_536, 65_537))
def test_long_run_key_layout_at_65536_runs(gpu, long_runs):
    """(b, k) = (16, 6) and (17, 5) at N = 17: 16.8 M rows, built and checked on the device; the second long round reads
    past N; bytes_keys_kernel, long_rows_kernel and both slot kernels make 17 trips"""
    import torch
    N = 17
    b, k = H.LAYOUT_LONG_RUNS[long_runs]
    lengths, kinds, dups = H.layout_tensors(torch, long_runs, "cuda")
    case = H.bytes_round_rows(torch, lengths, kinds, N, k, seed=long_runs, device="cuda", dups=dups)
    first = H.bytes_first_round(lengths.cpu().numpy(), N)
    assert (first["long_runs"], first["b"], first["k"], first["long_trips"]) == (long_runs, b, k, 17)
    assert case["n"] == 257 * long_runs and not torch.equal(case["rows"], case["sorted"])
    _check_on_device(gpu, case)


# ---- d. short-run grid stride --------------------------------------------------------------------------------------------------

def test_short_runs_second_trip(gpu):
    """4 200 000 runs of two rows and 2 000 runs of 65 ... 256 rows, N = 17, decided in the last byte: more than 2^20
    workgroups of four runs, so short_runs_kernel's loop, with its barriers, makes a second trip"""
    import torch
    N = 17
    lengths, kinds, dups = H.stride_tensors(torch, "cuda")
    case = H.bytes_round_rows(torch, lengths, kinds, N, 8, seed=4, device="cuda", dups=dups)
    first = H.bytes_first_round(lengths.cpu().numpy(), N)
    assert first["short_trips"] == 2 and first["long_runs"] == 0 and first["runs"] == H.STRIDE_PAIRS + H.STRIDE_MID
    assert not torch.equal(case["rows"], case["sorted"])
    _check_on_device(gpu, case)


# ---- e. stability, records form ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", H.RANK_WIDTHS)
def test_records_keep_input_order_in_short_runs(gpu, N):
    _check_records(gpu, _case("ranking", N), seed=1000 + N)


@pytest.mark.parametrize("N,short,long", H.BUDGET_PAIRS)
def test_records_keep_input_order_at_the_staging_budget(gpu, N, short, long):
    _check_records(gpu, _case("budget", N, short, long), seed=2000 + N)


@pytest.mark.parametrize("long_runs,N", LAYOUT_SMALL)
def test_records_keep_input_order_through_long_rounds(gpu, long_runs, N):
    """runs of 257 records of which a third carry equal keys: they survive every pair-sort round in input order"""
    _check_records(gpu, _case("layout", long_runs, N), seed=3000 + long_runs * 100 + N)


# ---- f. the widened route (N <= 16) past its grid cap -------------------------------------------------------------------------

@pytest.mark.parametrize("N", (3, 11, 16))
def test_widened_route_past_its_grid_cap(gpu, N):
    """2^20 + 3 rows: bytes_expand_kernel and bytes_compact_kernel make a second trip (their grid covers 4 096 x 256 rows)"""
    import torch
    n = H.GRID_ROWS + 3
    rng = np.random.default_rng(0xF00 + N)
    a = rng.integers(0, 256, size=(n, N), dtype=np.uint8)
    a[rng.random((n, N)) < 0.3] = 0
    a[1::7] = a[0::7][: a[1::7].shape[0]]
    want = _sorted_by_numpy(a)
    t = torch.from_numpy(a).cuda()
    gpu.sort_bytes_device_tensor(t)
    assert np.array_equal(t.cpu().numpy(), want), "device entry"
    host = a.copy()
    gpu.sort_host_array(host, key="bytes")
    assert np.array_equal(host, want), "host entry"
    gpu.device_status()
