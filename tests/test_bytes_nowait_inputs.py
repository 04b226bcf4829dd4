"""The round loop of the nowait [u8; N] route (bytes_order_nowait, rdst_amd/csrc/rdst_bytes.hip) restated
in numpy and checked against a stable lexicographic order, and the inputs of tests/test_gpu_bytes_nowait.py shown to leave
the tie flag down or to raise it as each is meant to, so that the GPU tests are known to reach both branches."""
import os
import re

import numpy as np
import pytest

import bytes_nowait_inputs as B
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("random",) + B.FLAG_UP_FAMILIES


def _source():
    with open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_bytes.hip")) as f:
        return f.read()


def test_constants_are_the_library_s():
    src = _source()
    assert re.search(r"constexpr uint32_t GRID_CAP = 256 \* 16;", src)
    assert B.GRID_ROWS == H.GRID_ROWS == 256 * 16 * 256
    assert "int bytes_order_nowait(" in src and "tie_flag_kernel" in src and "chunk_keys_kernel" in src
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    assert f"#define RDST_BYTES_NOWAIT_MAX_N {B.NOWAIT_MAX_N}u" in header
    assert max(B.WIDE_WIDTHS) == B.NOWAIT_MAX_N and -(-B.NOWAIT_MAX_N // 8) == 16


@pytest.mark.parametrize("N", B.CPU_WIDTHS)
@pytest.mark.parametrize("name", FAMILIES)
def test_round_loop_is_the_stable_lexicographic_order(name, N):
    """prefix sort, flag, C rounds (constant keys when the flag is down): the stable order of the whole rows"""
    for n in B.CPU_LENGTHS:
        rows = B.family(name, n, N)
        idx, flag = B.nowait_order(rows)
        assert np.array_equal(idx, B.stable_order(rows)), (name, n, N)
        assert flag == (name != "random"), (name, n, N)


@pytest.mark.parametrize("N", B.WIDE_WIDTHS)
def test_gpu_families_raise_or_leave_the_flag(N):
    """at the GPU tests' own row counts: random rows have no two equal 8-byte prefixes (flag down: the route's result then
    rests on the prefix sort alone), every other family ties some"""
    for n in B.lengths(H.pair_tile(8, 4)):
        prefix = np.sort(B.chunk_keys(B.family("random", n, N), 0))
        assert (prefix[1:] != prefix[:-1]).all(), (n, N)
        for name in B.FLAG_UP_FAMILIES:
            rows = B.family(name, n, N)
            prefix = np.sort(B.chunk_keys(rows, 0))
            assert (prefix[1:] == prefix[:-1]).any(), (name, n, N)
            if n >= 300 and name != "all equal":
                assert len(np.unique(rows, axis=0)) >= 3, (name, n, N)        # the rounds have something to order


def test_flag_up_families_need_the_rounds():
    """in every flag-up family with distinct rows the prefix sort alone leaves the rows out of order"""
    for name in ("last byte", "middle chunk", "three rows"):
        for N in B.WIDE_WIDTHS:
            rows = B.family(name, 300, N)
            by_prefix = np.argsort(B.chunk_keys(rows, 0), kind="stable")
            assert not np.array_equal(rows[by_prefix], rows[B.stable_order(rows)]), (name, N)


@pytest.mark.parametrize("n,pos", ((300, 0), (300, 255), (300, 298), (5_377, 255), (5_377, 256), (5_377, 4_095)))
def test_one_pair_is_what_it_says(n, pos):
    """distinct prefixes but for the sorted positions pos and pos + 1; the prefix sort alone leaves that pair the wrong way
    round; the restated loop mends it"""
    for N in (17, 25):
        rows, srt = B.one_pair(n, N, pos)
        prefix = B.chunk_keys(srt, 0)
        same = np.flatnonzero(prefix[1:] == prefix[:-1])
        assert same.tolist() == [pos] and (prefix[1:] >= prefix[:-1]).all()
        assert np.array_equal(rows[B.stable_order(rows)], srt)
        by_prefix = rows[np.argsort(B.chunk_keys(rows, 0), kind="stable")]
        wrong = np.flatnonzero((by_prefix != srt).any(axis=1))
        assert wrong.tolist() == [pos, pos + 1]
        idx, flag = B.nowait_order(rows)
        assert flag and np.array_equal(rows[idx], srt)


@pytest.mark.parametrize("L", sorted(B.FIELD_TABLES))
@pytest.mark.parametrize("record_bytes", B.RECORD_SIZES)
def test_record_tables(record_bytes, L):
    """every table adds up to its L, fits the record in front of the payload, and its cases hold equal keys (stability shows)
    and tied prefixes (the rounds run); the tables together mix every kind, a byte string and a descending field"""
    fields = B.field_table(L, record_bytes)
    assert sum(f[1] for f in fields) == L and len(fields) <= 16
    assert all(f[0] + f[1] <= record_bytes - 4 for f in fields)
    raw, _fields, exp = B.record_case(300, record_bytes, L)
    k = B.kmatrix(raw, fields)
    assert k.shape == (300, L)
    assert len(np.unique(k, axis=0)) < 300 - 50                      # equal keys: the payload tells input order
    if L > 8:
        idx, flag = B.nowait_order(k)
        assert flag and np.array_equal(raw[idx], exp)
    seq = exp[:, record_bytes - 4:].copy().view("<u4").ravel()
    ke = B.kmatrix(exp, fields)
    tied = (ke[1:] == ke[:-1]).all(axis=1)
    assert tied.any() and (seq[1:][tied] > seq[:-1][tied]).all()


def test_record_tables_mix_the_kinds():
    for L in (9, 12, 16, 17, 40, 128):
        assert L in B.FIELD_TABLES
    wide = [f for L, t in B.FIELD_TABLES.items() if L > 8 for f in t]
    assert {f[2] for f in wide} == {B.UNSIGNED, B.SIGNED, B.FLOAT, B.BYTES_BE}
    assert any(f[3] for f in wide) and any(f[2] == B.FLOAT and f[1] == 4 for f in wide) and any(f[2] == B.FLOAT and f[1] == 8 for f in wide)
    assert 256 * 24 <= 32768 < 256 * 130                              # PACK_TILE x R against PACK_LDS_BYTES: staged, direct
    src = _source()
    assert "constexpr uint32_t PACK_TILE = 256;" in src and "constexpr uint32_t PACK_LDS_BYTES = 32768;" in src
