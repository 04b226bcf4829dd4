"""The nowait entries for wide keys on the device (rdst_hip_sort_bytes_device_nowait,
rdst_hip_sort_records_by_fields_device_nowait): every result is compared byte for byte with the blocking
twin's on a copy and with numpy.  The row counts sit around the pair sort's tile, the widths at the chunk borders of the
round loop; random rows leave the tie flag down, every other family raises it (tests/test_bytes_nowait_inputs.py shows
both on the CPU)."""
import ctypes

import numpy as np
import pytest

import bytes_nowait_inputs as B
import helpers as H

pytestmark = pytest.mark.gpu

ARG = -1
LENGTHS = B.lengths(H.pair_tile(8, 4))


def F(fields):
    from rdst_amd import KeyField
    return [KeyField(o, b, k, bool(d)) for o, b, k, d in fields]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()         # (a copy: the shared cases are read-only)


def _rows_sorted(a):
    """whole rows are the key: equal rows are indistinguishable, any lexicographic sort is THE answer"""
    n, N = a.shape
    return np.sort(np.ascontiguousarray(a).view(f"V{N}").ravel()).view(np.uint8).reshape(n, N)


def _check_rows(gpu, rows, what, want=None):
    want = _rows_sorted(rows) if want is None else want
    t = _dev(rows)
    gpu.sort_bytes_device_nowait_tensor(t)
    got = t.cpu().numpy()
    twin = _dev(rows)
    gpu.sort_bytes_device_tensor(twin)
    assert np.array_equal(got, twin.cpu().numpy()), (what, "against the blocking entry")
    assert np.array_equal(got, want), (what, "against numpy")


def _check_records(gpu, raw, fields, exp, what):
    t = _dev(raw)
    gpu.sort_records_device_nowait_tensor(t, F(fields))
    got = t.cpu().numpy()
    twin = _dev(raw)
    gpu.sort_records_device_tensor(twin, F(fields))
    assert np.array_equal(got, twin.cpu().numpy()), (what, "against the blocking entry")
    assert np.array_equal(got, exp), (what, "against numpy")


# ---- chunk borders, flag down and flag up -------------------------------------------------------------------------------

@pytest.mark.parametrize("N", B.WIDE_WIDTHS)
def test_random_rows_leave_the_flag_down(gpu, N):
    """no two 8-byte prefixes collide: every round's keys are 0, the order is the prefix sort's"""
    for n in LENGTHS:
        _check_rows(gpu, B.family("random", n, N), f"random n={n} N={N}")
    gpu.device_status()


@pytest.mark.parametrize("N", B.WIDE_WIDTHS)
@pytest.mark.parametrize("name", B.FLAG_UP_FAMILIES)
def test_tied_prefixes_raise_the_flag(gpu, name, N):
    """one family per test: rows that differ in the last byte only, inside a middle chunk only, not at all, three rows repeated"""
    for n in LENGTHS:
        _check_rows(gpu, B.family(name, n, N), f"{name} n={n} N={N}")
    gpu.device_status()


@pytest.mark.parametrize("N", B.FORWARDED_WIDTHS)
def test_narrow_rows_are_forwarded(gpu, N):
    for n in LENGTHS:
        for name in ("random", "last byte", "three rows"):
            _check_rows(gpu, B.family(name, n, N), f"{name} n={n} N={N}")
    gpu.device_status()


@pytest.mark.parametrize("n,pos", ((300, 255), (70_001, 255), (70_001, 69_999), (B.GRID_ROWS + 3, 255), (B.GRID_ROWS + 3, B.GRID_ROWS - 1),
                                   (B.GRID_ROWS + 3, B.GRID_ROWS)))
def test_one_equal_pair_is_seen_wherever_it_lies(gpu, n, pos):
    """distinct prefixes but for the sorted positions pos and pos + 1, which the prefix sort leaves the wrong way round:
    across the border of two workgroups of the tie kernel (255 | 256), the last pair, and the last pair of the kernel's first
    grid trip and the first of its second (n just past GRID_CAP x 256)"""
    rows, srt = B.one_pair(n, 17, pos, seed=1)
    _check_rows(gpu, rows, f"one pair at {pos} of {n}", want=srt)
    gpu.device_status()


# ---- records ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("record_bytes", B.RECORD_SIZES)
@pytest.mark.parametrize("L", (9, 12, 16, 17, 40, 128))
def test_records_by_described_keys(gpu, L, record_bytes):
    """unsigned, signed, f32 / f64, byte-string and descending fields; 24-byte records (the staged pack) and 130-byte
    records (the direct pack); half of the records share their keys with others and keep their input order"""
    for n in (3, 300, H.pair_tile(8, 4) + 1, 70_001):
        raw, fields, exp = B.record_case(n, record_bytes, L)
        _check_records(gpu, raw, fields, exp, f"L={L} R={record_bytes} n={n}")
    gpu.device_status()


@pytest.mark.parametrize("record_bytes", B.RECORD_SIZES)
@pytest.mark.parametrize("L", (9, 40, 128))
def test_records_with_equal_keys_keep_their_input_order(gpu, L, record_bytes):
    raw, fields, exp = B.record_case(70_001, record_bytes, L, True)
    assert np.array_equal(exp, raw) and len(np.unique(B.kmatrix(raw, fields), axis=0)) == 1
    _check_records(gpu, raw, fields, exp, f"equal keys L={L} R={record_bytes}")
    gpu.device_status()


@pytest.mark.parametrize("record_bytes", B.RECORD_SIZES)
def test_short_described_keys_are_forwarded(gpu, record_bytes):
    for n in (3, 300, 70_001):
        raw, fields, exp = B.record_case(n, record_bytes, 8)
        _check_records(gpu, raw, fields, exp, f"L=8 R={record_bytes} n={n}")
    gpu.device_status()


# ---- unaligned rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (17, 25, 127))
@pytest.mark.parametrize("offset", (1, 2, 4))
def test_unaligned_rows(gpu, N, offset):
    """the row base 1, 2 and 4 bytes past a 16-byte boundary, N odd: load_be's word loads never apply to every row"""
    import torch
    for name in ("random", "middle chunk"):
        for n in (300, 70_001):
            rows = B.family(name, n, N, seed=offset)
            buf = torch.zeros(n * N + 512, dtype=torch.uint8, device="cuda")
            start = (-buf.data_ptr()) % 256 + offset
            t = buf[start:start + n * N].view(n, N)
            assert t.data_ptr() % 16 == offset
            t.copy_(torch.from_numpy(rows))
            gpu.sort_bytes_device_nowait_tensor(t)
            assert np.array_equal(t.cpu().numpy(), _rows_sorted(rows)), (name, n, N, offset)
            assert not buf[:start].any() and not buf[start + n * N:].any()
    gpu.device_status()


# ---- bounds ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (17, 128))
@pytest.mark.parametrize("name", ("random", "last byte"))
def test_rows_and_scratch_stay_inside_their_bands(gpu, name, N):
    """rows one byte past a 256-byte boundary, a scratch of exactly rdst_hip_sort_bytes_scratch_bytes, bands around both"""
    from rdst_amd import _lib
    lib = _lib.load()
    n = 70_001
    rows = B.family(name, n, N, seed=3)
    need = int(lib.rdst_hip_sort_bytes_scratch_bytes(n, N))
    rb = H.banded((n, N), np.uint8, offset_bytes=1, seed=1, init=rows, name="rows")
    sb = H.banded((need,), np.uint8, seed=2, name="scratch")
    assert rb["rows"].data_ptr() % 256 == 1 and sb["scratch"].data_ptr() % 256 == 0
    gpu.sort_bytes_device_nowait_tensor(rb["rows"], sb["scratch"])
    assert np.array_equal(rb["rows"].cpu().numpy(), _rows_sorted(rows))
    rb.check(f"rows {name} N={N}")
    sb.check(f"scratch {name} N={N}")


@pytest.mark.parametrize("L,record_bytes", ((17, 24), (128, 130)))
def test_records_and_scratch_stay_inside_their_bands(gpu, L, record_bytes):
    from rdst_amd import _lib
    from rdst_amd.radix_sort import _field_table
    n = 70_001
    raw, fields, exp = B.record_case(n, record_bytes, L)
    need = int(_lib.load().rdst_hip_sort_records_by_fields_scratch_bytes(n, record_bytes, *_field_table(F(fields))))
    rb = H.banded((n, record_bytes), np.uint8, offset_bytes=1, seed=3, init=np.array(raw), name="records")
    sb = H.banded((need,), np.uint8, seed=4, name="scratch")
    gpu.sort_records_device_nowait_tensor(rb["records"], F(fields), sb["scratch"])
    assert np.array_equal(rb["records"].cpu().numpy(), exp)
    rb.check(f"records L={L}")
    sb.check(f"scratch L={L}")


def test_a_scratch_one_byte_short_is_refused(gpu):
    import torch
    from rdst_amd import _lib
    from rdst_amd.radix_sort import _field_table
    lib = _lib.load()
    n, N = 300, 24
    rows = B.family("random", n, N)
    t = _dev(rows)
    need = int(lib.rdst_hip_sort_bytes_scratch_bytes(n, N))
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.rdst_hip_sort_bytes_device_nowait(ctypes.c_void_p(t.data_ptr()), n, N, ctypes.c_void_p(scratch.data_ptr()), need - 1, s) == ARG
    raw, fields, _exp = B.record_case(n, 24, 17)
    table, nf = _field_table(F(fields))
    need = int(lib.rdst_hip_sort_records_by_fields_scratch_bytes(n, 24, table, nf))
    r = _dev(raw)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
    assert lib.rdst_hip_sort_records_by_fields_device_nowait(ctypes.c_void_p(r.data_ptr()), n, 24, table, nf, ctypes.c_void_p(scratch.data_ptr()),
                                                             need - 1, s) == ARG
    gpu.device_status()
    assert np.array_equal(t.cpu().numpy(), rows) and np.array_equal(r.cpu().numpy(), raw) and not scratch.any()


# ---- stream order ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("random", "last byte"))
def test_the_call_takes_its_place_in_stream_order(gpu, name):
    """the rows are produced by torch ops on a side stream; the nowait call (check=False) and the copy to pinned host memory
    are enqueued behind them on that stream with no host synchronisation in between"""
    import torch
    from rdst_amd import _lib
    n, N = 70_001, 32
    rows = B.family(name, n, N, seed=9)
    source = _dev((rows ^ 0x5A)[::-1])
    scratch = torch.empty(int(_lib.load().rdst_hip_sort_bytes_scratch_bytes(n, N)), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, N), dtype=torch.uint8).pin_memory()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t = (source.flip(0) ^ 0x5A).contiguous()          # the producer: the rows exist only in stream order
        gpu.sort_bytes_device_nowait_tensor(t, scratch, check=False)
        out.copy_(t, non_blocking=True)
    side.synchronize()
    assert np.array_equal(out.numpy(), _rows_sorted(rows))
    with torch.cuda.stream(side):
        gpu.device_status()


def test_records_take_their_place_in_stream_order(gpu):
    import torch
    n, record_bytes, L = 70_001, 24, 17
    raw, fields, exp = B.record_case(n, record_bytes, L)
    source = _dev(raw ^ 0xA5)
    out = torch.empty((n, record_bytes), dtype=torch.uint8).pin_memory()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t = source ^ 0xA5
        gpu.sort_records_device_nowait_tensor(t, F(fields), check=False)
        out.copy_(t, non_blocking=True)
    side.synchronize()
    assert np.array_equal(out.numpy(), exp)
    with torch.cuda.stream(side):
        gpu.device_status()
