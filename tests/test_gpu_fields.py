"""Records ordered by a described key (rdst_key_field tables) on the device: rdst_hip_sort_records_by_fields (host slice)
and rdst_hip_sort_records_by_fields_device (in place), through the Python mirror.  The expected order is numpy's: the K
matrix of mapped key bytes built from the raw record bytes, then a stable np.lexsort; whole records are compared row for
row (the route is stable, so the comparison is exact)."""
import ctypes
import json
import os

import numpy as np
import pytest

from helpers import Bands, banded, mapped_key, random_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
LENGTHS = (2, 3, 255, 256, 257, 4097, 100_003)   # 4097: one past the scan tile; 100 003: past the one-workgroup pair sort
WIDTHS = (1, 2, 4, 5, 8, 9, 16, 17, 24)


def F(offset, nbytes, kind, descending=False):
    from rdst_amd import KeyField
    return KeyField(offset, nbytes, kind, descending)


def kmatrix(raw, fields):
    """K of every record, (n, L) uint8: the fields' mapped values, big-endian, in field order"""
    cols = []
    for f in fields:
        b = raw[:, f.offset:f.offset + f.bytes].copy()
        if f.kind != BYTES_BE:
            b = b[:, ::-1].copy()                     # stored little-endian
            if f.kind == SIGNED:
                b[:, 0] ^= 0x80
            elif f.kind == FLOAT:
                neg = (b[:, 0] & 0x80) != 0
                b[neg] = ~b[neg]
                b[~neg, 0] ^= 0x80
        if f.descending:
            b = ~b
        cols.append(b)
    return np.concatenate(cols, axis=1)


def expected(raw, fields):
    k = kmatrix(raw, fields)
    return raw[np.lexsort(k.T[::-1])]


def host_sorted(gpu, raw, fields):
    got = raw.copy()
    gpu.sort_host_records(got.view(np.dtype([("b", "u1", (raw.shape[1],))])).reshape(-1), fields)
    return got


def device_sorted(gpu, raw, fields, base_offset=0):
    import torch
    n, rec = raw.shape
    buf = torch.zeros(n * rec + 512, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 256 + base_offset
    t = buf[start:start + n * rec].view(n, rec)
    assert t.data_ptr() % 256 == base_offset
    t.copy_(torch.from_numpy(raw))
    gpu.sort_records_device_tensor(t, fields)
    return t.cpu().numpy()


def check_both(gpu, raw, fields, what, exp=None):
    exp = expected(raw, fields) if exp is None else exp
    assert np.array_equal(host_sorted(gpu, raw, fields), exp), (what, "host")
    assert np.array_equal(device_sorted(gpu, raw, fields), exp), (what, "device")


def records(rng, n, rec, tie_cols=()):
    """random rows; the columns in tie_cols take few values, so that later key bytes decide"""
    raw = rng.integers(0, 256, size=(n, rec), dtype=np.uint8)
    for c in tie_cols:
        raw[:, c] &= 0x81
    return raw


def descriptions(L):
    """a one-field and a two-field description of an L-byte key inside 32-byte records, at odd offsets"""
    one = {1: F(5, 1, UNSIGNED), 2: F(5, 2, SIGNED), 4: F(5, 4, FLOAT), 8: F(5, 8, SIGNED), 16: F(5, 16, UNSIGNED)}.get(L, F(5, L, BYTES_BE))
    two = {1: None, 2: [F(9, 1, SIGNED), F(3, 1, UNSIGNED)], 4: [F(9, 2, UNSIGNED), F(3, 2, SIGNED)], 5: [F(9, 1, UNSIGNED), F(3, 4, FLOAT)],
           8: [F(11, 4, SIGNED), F(3, 4, UNSIGNED)], 9: [F(1, 1, SIGNED), F(3, 8, FLOAT)], 16: [F(19, 8, UNSIGNED), F(3, 8, SIGNED)],
           17: [F(1, 1, UNSIGNED), F(3, 16, SIGNED)], 24: [F(23, 8, FLOAT), F(3, 16, UNSIGNED)]}[L]
    return [[one]] + ([two] if two else [])


def test_pack_kernel_writes_k(gpu):
    """pack_fields_kernel alone (rdst_hip_pack_fields_device): every form of K, staged through LDS (small records) and read
    directly (records of 200 bytes), a partial last tile, and the grid-stride loop's second trip at 2^20 + 3 records"""
    import torch
    from rdst_amd import _lib
    from rdst_amd.radix_sort import _field_table
    lib = _lib.load()
    rng = np.random.default_rng(1)
    cases = [(1000, 13, [F(12, 1, UNSIGNED), F(3, 2, SIGNED, True)]), (1000, 200, [F(195, 4, FLOAT)]),
             (777, 37, [F(1, 4, FLOAT, True), F(33, 4, SIGNED)]), (777, 200, [F(191, 8, FLOAT), ]),
             (1001, 37, [F(1, 16, SIGNED), F(20, 17, BYTES_BE, True), F(7, 4, FLOAT)]), (300, 200, [F(3, 8, SIGNED), F(100, 100, BYTES_BE)]),
             ((1 << 20) + 3, 16, [F(3, 1, UNSIGNED), F(7, 2, SIGNED)]), ((1 << 20) + 3, 16, [F(3, 1, UNSIGNED), F(7, 4, FLOAT)]),
             ((1 << 20) + 3, 16, [F(0, 1, SIGNED), F(7, 8, FLOAT, True)])]
    for n, rec, fields in cases:
        raw = records(rng, n, rec)
        k = kmatrix(raw, fields)
        L = k.shape[1]
        width = 4 if L <= 4 else 8 if L <= 8 else L
        t = torch.from_numpy(raw).cuda()
        keys = torch.zeros(n * width, dtype=torch.uint8, device="cuda")
        rows = torch.zeros(n, dtype=torch.int32, device="cuda")
        table, nf = _field_table(fields)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.rdst_hip_pack_fields_device(ctypes.c_void_p(t.data_ptr()), n, rec, table, nf, ctypes.c_void_p(keys.data_ptr()),
                                                   ctypes.c_void_p(rows.data_ptr()), s))
        gpu.device_status()
        got = keys.cpu().numpy().reshape(n, width)
        if L <= 8:
            want = np.zeros((n, width), dtype=np.uint8)
            want[:, :L] = k
            want = want[:, ::-1]                       # the integer key, little-endian in memory
            assert np.array_equal(rows.cpu().numpy(), np.arange(n, dtype=np.int32)), (n, rec, L)
        else:
            want = k
        assert np.array_equal(got, want), (n, rec, L)


@pytest.mark.parametrize("L", WIDTHS)
def test_key_widths(gpu, L):
    rng = np.random.default_rng(0xF1E1D + L)
    for fields in descriptions(L):
        for n in LENGTHS:
            raw = records(rng, n, 32, tie_cols=(3, 4, 5, 6, 9, 11, 12, 23, 19) if n > 300 else (3, 5, 9, 11))
            check_both(gpu, raw, fields, (L, len(fields), n))


def test_second_trip_of_the_grid_stride_loop(gpu):
    n = (1 << 20) + 3
    rng = np.random.default_rng(20)
    raw = records(rng, n, 16, tie_cols=(0, 7, 8))
    fields = [F(0, 1, SIGNED), F(7, 8, FLOAT)]
    assert np.array_equal(device_sorted(gpu, raw, fields), expected(raw, fields))


def _specials(kind, width):
    """the values the key maps bend at, as (m, width) little-endian bytes"""
    if kind == FLOAT:
        ft, ut = f"<f{width}", f"<u{width}"
        top = 1 << (8 * width - 1)
        quiet = {4: 0x7FC00000, 8: 0x7FF8000000000000}[width]
        inf = {4: 0x7F800000, 8: 0x7FF0000000000000}[width]
        bits = [0, top, inf, inf | top, quiet, quiet | top, quiet | 1, quiet | top | 1, inf | 1, inf | top | 1, (top - 1), (2 * top - 1),
                1, top | 1]
        v = np.array(bits, dtype=ut).view(ft)
        assert np.isnan(v).sum() == 8
        return v.view(np.uint8).reshape(-1, width)
    vals = [-(1 << (8 * width - 1)), -1, 0, 1, (1 << (8 * width - 1)) - 1] if kind == SIGNED else [0, 1, (1 << (8 * width - 1)), (1 << (8 * width)) - 1]
    return np.array([list((v % (1 << (8 * width))).to_bytes(width, "little")) for v in vals], dtype=np.uint8)


def _order_by_mapped_key(values, kind, width):
    """stable order of (n, width) little-endian values by tests/helpers.mapped_key (128-bit: high limb mapped, low limb as is)"""
    if kind == BYTES_BE:
        return np.lexsort(values.T[::-1])
    letter = {UNSIGNED: "u", SIGNED: "i", FLOAT: "f"}[kind]
    if width == 16:
        low = np.ascontiguousarray(values[:, :8]).view("<u8").ravel()
        high = mapped_key(np.ascontiguousarray(values[:, 8:]).view(f"<{letter}8").ravel())
        return np.lexsort((low, high))
    return np.argsort(mapped_key(np.ascontiguousarray(values).view(f"<{letter}{width}").ravel()), kind="stable")


KINDS = [(UNSIGNED, w) for w in (1, 2, 4, 8, 16)] + [(SIGNED, w) for w in (1, 2, 4, 8, 16)] + [(FLOAT, 4), (FLOAT, 8)] + \
    [(BYTES_BE, w) for w in (1, 7, 8, 9, 33, 4096)]


@pytest.mark.parametrize("kind,width", KINDS)
def test_kinds_and_specials(gpu, kind, width):
    rng = np.random.default_rng(width * 4 + kind)
    n = 300 if width == 4096 else 3000
    rec = width + 5
    raw = records(rng, n, rec)
    if kind == BYTES_BE:
        raw[:, 3:3 + width][rng.random((n, width)) < 0.5] = 0
        raw[::4, 3:3 + width] = raw[1::4, 3:3 + width][: raw[::4].shape[0]]
    else:
        sp = _specials(kind, width)
        pick = rng.integers(0, len(sp), size=n)
        use = rng.random(n) < 0.5
        raw[use, 3:3 + width] = sp[pick[use]]
    values = raw[:, 3:3 + width]
    exp = raw[_order_by_mapped_key(values, kind, width)]
    fields = [F(3, width, kind)]
    assert np.array_equal(exp, expected(raw, fields))     # the two independent statements of the order agree
    check_both(gpu, raw, fields, (kind, width), exp)


def test_ties_and_significance(gpu):
    """3 values in the first field, 5 in the second: both the field order and stability show; then every key equal"""
    rng = np.random.default_rng(35)
    for n in (1000, 100_003):
        for fields in ([F(2, 1, UNSIGNED), F(5, 2, SIGNED)], [F(5, 2, SIGNED), F(2, 1, UNSIGNED)], [F(2, 1, UNSIGNED), F(5, 8, SIGNED)],
                       [F(5, 8, SIGNED), F(1, 2, UNSIGNED)]):
            raw = records(rng, n, 16)
            raw[:, 1:13] = 0
            raw[:, 2] = rng.choice(np.array([7, 130, 255], dtype=np.uint8), size=n)
            raw[:, 5] = rng.choice(np.array([0, 1, 127, 128, 255], dtype=np.uint8), size=n)
            raw[:, 6:13] = np.where(raw[:, 5:6] >= 128, 255, 0)      # sign-extended: the i64 takes the same five values
            exp = expected(raw, fields)
            check_both(gpu, raw, fields, (n, fields), exp)
            assert len(np.unique(kmatrix(raw, fields), axis=0)) == 15
    raw = records(rng, 5000, 16)
    raw[:, 4:14] = 9
    for fields in ([F(4, 4, FLOAT)], [F(4, 8, UNSIGNED)], [F(4, 2, SIGNED), F(6, 8, BYTES_BE)]):
        check_both(gpu, raw, fields, ("all equal", fields), raw)


def test_descending(gpu):
    rng = np.random.default_rng(44)
    n = 20_000
    raw = records(rng, n, 48, tie_cols=(1, 2, 3, 4, 9))
    raw[: n // 2, 1:5] = random_bits(n // 2, "float32", seed=3).view(np.uint8).reshape(-1, 4)   # NaNs, infinities, both zeros
    for d0 in (False, True):
        for d1 in (False, True):
            for fields in ([F(9, 1, UNSIGNED, d0), F(12, 2, SIGNED, d1)], [F(1, 4, FLOAT, d0), F(9, 4, SIGNED, d1)],
                           [F(9, 1, SIGNED, d0), F(1, 4, FLOAT, d1)], [F(1, 4, FLOAT, d0), F(20, 17, BYTES_BE, d1)],
                           [F(9, 1, UNSIGNED, d0), F(20, 3, BYTES_BE, d1)]):
                check_both(gpu, raw, fields, fields)
    # a descending single field is the ascending order reversed run by run: the keys are non-increasing
    got = host_sorted(gpu, raw, [F(9, 4, SIGNED, True)])
    v = np.ascontiguousarray(got[:, 9:13]).view("<i4").ravel()
    assert (v[1:] <= v[:-1]).all()


@pytest.mark.parametrize("rec", (4, 13, 16, 37, 64, 200))
def test_layouts(gpu, rec):
    """odd offsets, overlapping fields, a field that ends on the record's last byte, record bases 1 and 4 bytes past an aligned
    address; 200-byte records take the direct-read form of the pack kernel"""
    rng = np.random.default_rng(rec)
    last4 = rec - 4
    tables = [[F(rec - 1, 1, UNSIGNED)], [F(1, 2, SIGNED), F(rec - 2, 2, UNSIGNED)], [F(last4, 4, FLOAT), F(1, 3, BYTES_BE)],
              [F(1, 2, UNSIGNED), F(0, 4, SIGNED)]]                                   # the last: overlapping fields
    if rec >= 13:
        tables += [[F(5, 8, SIGNED)], [F(rec - 8, 8, FLOAT, True), F(1, 1, SIGNED)], [F(1, 8, UNSIGNED), F(3, 9, BYTES_BE)]]
    if rec >= 37:
        tables += [[F(rec - 16, 16, SIGNED), F(1, 8, FLOAT)], [F(3, rec - 3, BYTES_BE)]]
    for fields in tables:
        for n in (257, 5000):
            raw = records(rng, n, rec, tie_cols=(1, 2, rec - 1, rec - 2))
            exp = expected(raw, fields)
            assert np.array_equal(host_sorted(gpu, raw, fields), exp), (rec, fields, n, "host")
            for base in (0, 1, 4):
                assert np.array_equal(device_sorted(gpu, raw, fields, base), exp), (rec, fields, n, base)


def test_single_field_equals_the_single_field_entry(gpu):
    rng = np.random.default_rng(66)
    n = 50_000
    for key in ("<u4", "<f8", ("u1", (20,))):
        dt = np.dtype([("k", *key) if isinstance(key, tuple) else ("k", key), ("seq", "<u8")])
        a = np.zeros(n, dtype=dt)
        kb = dt.fields["k"][0].itemsize
        raw = a.view(np.uint8).reshape(n, dt.itemsize)
        raw[:, :kb] = rng.integers(0, 256, size=(n, kb), dtype=np.uint8)
        raw[:, 1:kb - 1] &= 0x80                  # ties
        a["seq"] = np.arange(n)
        b = a.copy()
        gpu.sort_host_records(a, "k")
        gpu.sort_host_records(b, ["k"])
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), key
        assert not np.array_equal(a["seq"], np.arange(n))


@pytest.mark.parametrize("fields_of", (lambda: [F(3, 4, FLOAT)], lambda: [F(1, 2, UNSIGNED), F(7, 4, SIGNED), F(20, 2, BYTES_BE)],
                                       lambda: [F(1, 8, SIGNED), F(19, 16, UNSIGNED)]), ids=("L4", "L8", "L24"))
def test_guard_bands(gpu, fields_of):
    """records one byte past a 256-byte boundary with bands on both sides, the scratch exactly as long as the size call
    says, with bands on both sides: nothing outside the records changes; the host entry leaves the bytes around the
    caller's array alone"""
    import torch
    from rdst_amd import _lib
    from rdst_amd.radix_sort import _field_table
    fields = fields_of()
    lib = _lib.load()
    rng = np.random.default_rng(77)
    n, rec = 70_001, 37
    raw = records(rng, n, rec, tie_cols=(1, 2, 3, 4, 7, 8))
    exp = expected(raw, fields)
    table, nf = _field_table(fields)
    need = int(lib.rdst_hip_sort_records_by_fields_scratch_bytes(n, rec, table, nf))
    assert need % 256 == 0
    bands = Bands([("scratch", ((need,), np.uint8), 0), ("records", raw, 257)], seed=9)
    assert bands["scratch"].data_ptr() % 256 == 0 and bands["records"].data_ptr() % 256 == 1
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rdst_hip_sort_records_by_fields_device(ctypes.c_void_p(bands["records"].data_ptr()), n, rec, table, nf,
                                                          ctypes.c_void_p(bands["scratch"].data_ptr()), need, s))
    gpu.device_status()
    bands.check("device entry")
    assert np.array_equal(bands["records"].cpu().numpy(), exp)
    host = banded((n, rec), np.uint8, offset_bytes=3, seed=10, device=None, init=raw)
    opts = _lib.HipOptsC(-1, 0, 0)
    _lib.check(lib.rdst_hip_sort_records_by_fields(ctypes.c_void_p(host["keys"].ctypes.data), n, rec, table, nf, ctypes.byref(opts)))
    host.check("host entry")
    assert np.array_equal(host["keys"], exp)


def test_error_word_stops_the_host_entry(gpu):
    import torch
    from rdst_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(88)
    raw = records(rng, 10_000, 24)
    for fields in ([F(1, 4, SIGNED)], [F(1, 2, UNSIGNED), F(8, 8, SIGNED)]):
        _lib.check(lib.rdst_hip_debug_raise_device_error(2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        got = raw.copy()
        with pytest.raises(_lib.RdstHipError) as e:
            gpu.sort_host_records(got.view(np.dtype([("b", "u1", (24,))])).reshape(-1), fields)
        assert e.value.code == -5
        assert np.array_equal(got, raw)
        gpu.device_status()                               # reported once: clean again
        check_both(gpu, raw, fields, fields)


def test_reference_example_orders(gpu):
    """examples/impl_radix_key.rs: the same four-byte struct by all bytes, by the even bytes, by the odd bytes"""
    with open(os.path.join(ROOT, "tests", "golden", "impl_radix_key_example.json")) as f:
        golden = json.load(f)
    assert [c["name"] for c in golden["cases"]] == ["all bytes", "even bytes", "odd bytes"]
    for case in golden["cases"]:
        raw = np.array(case["input"], dtype=np.uint8)
        printed = np.array(case["printed"], dtype=np.uint8)
        fields = [F(o, b, k, bool(fl)) for o, b, k, fl in case["fields"]]
        assert sum(f.bytes for f in fields) == case["levels"]
        assert np.array_equal(host_sorted(gpu, raw, fields), printed), case["name"]
        assert np.array_equal(device_sorted(gpu, raw, fields), printed), case["name"]
    raw = np.array(golden["cases"][0]["input"], dtype=np.uint8)
    assert np.array_equal(host_sorted(gpu, raw, [F(0, 4, BYTES_BE)]), np.array(golden["cases"][0]["printed"], dtype=np.uint8))
