"""The answers the C ABI's entry points give before their first HIP call: return code, a distinguishing piece of
rdst_hip_last_error(), and, where two checks could both fire, which one wins.  No device is touched: every pointer that
stands for device memory is a number that is never followed, and no call here gets past its checks.  (The answers that
come after an entry's first HIP call are in test_gpu_entries.py.)"""
import ctypes

import pytest

OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
U, S, F, BYTES_BE = 0, 1, 2, 3
P = 0x7F0000001000        # stands for an aligned device (or host) address; never followed
ODD = P + 2               # not aligned to 4 or 8 bytes
MAX_N = 4096              # RDST_BYTES_MAX_N


@pytest.fixture()
def call(hiplib):
    def go(name, *args, code, text=None):
        rc = getattr(hiplib, name)(*args)
        assert rc == code, (name, args, rc, hiplib.rdst_hip_last_error())
        if text is not None:
            assert text.encode() in hiplib.rdst_hip_last_error(), (name, args, hiplib.rdst_hip_last_error())
    return go


NULL_TMP, ODD_TMP = "null tmp pointer", "tmp pointer not aligned to the element size"
NULL_DST, ODD_DST = "null dst pointer", "dst pointer not aligned to the element size"
SCRATCH = "the scratch must hold at least 65536 elements"


def test_sort_device_second_buffer(call):
    e = "rdst_hip_sort_device"
    call(e, P, None, 8, 4, U, 4, None, code=ARG, text=NULL_TMP)
    call(e, P, ODD, 8, 4, U, 4, None, code=ALIGN, text=ODD_TMP)
    call(e, P, P + 4, 8, 8, U, 8, None, code=ALIGN, text=ODD_TMP)           # aligned to 4, not to the 8-byte element
    call(e, None, None, 8, 4, U, 4, None, code=ARG, text="null key pointer")  # the key checks come first
    call(e, ODD, None, 8, 4, U, 4, None, code=ALIGN, text="key pointer not aligned")
    call(e, P, None, 8, 4, U, 3, None, code=ARG, text="levels must equal")
    call(e, P, None, 1, 4, U, 4, None, code=OK)                             # len <= 1 needs no second buffer
    call(e, None, None, 0, 4, U, 4, None, code=OK)


def test_sort_device_lowmem_second_buffer_and_scratch(call):
    e = "rdst_hip_sort_device_lowmem"
    call(e, P, 100_000, 4, U, 4, None, 65536, None, code=ARG, text=NULL_TMP)
    call(e, P, 100_000, 4, U, 4, ODD, 65536, None, code=ALIGN, text=ODD_TMP)
    call(e, P, 100_000, 4, U, 4, P, 65535, None, code=ARG, text=SCRATCH)
    call(e, P, 100_000, 4, U, 4, P, 0, None, code=ARG, text=SCRATCH)
    call(e, P, 100_000, 4, U, 4, None, 65535, None, code=ARG, text=NULL_TMP)   # the pointer before its size
    call(e, P, 100_000, 4, U, 4, ODD, 65535, None, code=ALIGN, text=ODD_TMP)
    call(e, None, 100_000, 4, U, 4, None, 0, None, code=ARG, text="null key pointer")
    call(e, P, 1, 4, U, 4, None, 0, None, code=OK)                             # len <= 1: no scratch asked for
    call(e, None, 0, 4, U, 4, None, 0, None, code=OK)


def test_partition_device(call):
    e = "rdst_hip_partition_device"
    split = ctypes.c_uint64(7)
    sp = ctypes.byref(split)
    call(e, P, 100_000, 4, U, 4, 0, P, 65536, sp, None, code=ARG, text="level / digit out of range")
    call(e, P, 100_000, 4, U, 3, 256, P, 65536, sp, None, code=ARG, text="level / digit out of range")
    call(e, P, 100_000, 4, U, 0, 0, P, 65536, None, None, code=ARG, text="null split_out")
    call(e, P, 100_000, 4, U, 4, 0, P, 65536, None, None, code=ARG, text="level / digit out of range")  # before split_out
    call(e, P, 100_000, 4, U, 0, 0, None, 65536, None, None, code=ARG, text="null split_out")          # before tmp
    assert split.value == 7                                                   # nothing above wrote it
    call(e, P, 100_000, 4, U, 0, 0, None, 65536, sp, None, code=ARG, text=NULL_TMP)
    assert split.value == 0                                                   # zeroed once the arguments before it passed
    call(e, P, 100_000, 4, U, 0, 0, ODD, 65536, sp, None, code=ALIGN, text=ODD_TMP)
    call(e, P, 100_000, 4, U, 0, 0, P, 65535, sp, None, code=ARG, text=SCRATCH)
    call(e, P, 100_000, 4, U, 0, 0, None, 65535, sp, None, code=ARG, text=NULL_TMP)
    split.value = 7
    call(e, None, 0, 4, U, 0, 0, None, 0, sp, None, code=OK)                  # len == 0: split 0, no scratch asked for
    assert split.value == 0
    call(e, P, 1, 4, U, 0, 0, None, 65536, sp, None, code=ARG, text=NULL_TMP)  # one key is not a no-op here


def test_split_top16_device(call):
    e = "rdst_hip_split_top16_device"
    call(e, P, P, 8, 1, U, P, None, code=UNSUPPORTED, text="a 16-bit split needs keys of at least two bytes")
    call(e, P, P, 8, 1, U, None, None, code=UNSUPPORTED, text="a 16-bit split")    # the width before the counts pointer
    call(e, P, P, 8, 4, U, None, None, code=ARG, text="null counts pointer")
    call(e, P, None, 8, 4, U, None, None, code=ARG, text="null counts pointer")    # ... which comes before tmp
    call(e, None, P, 8, 4, U, P, None, code=ARG, text="null key pointer")


def test_scatter_level(call):
    e = "rdst_hip_scatter_level"
    counts = (ctypes.c_uint64 * 256)(*([9] * 256))
    call(e, P, P, 8, 4, U, 4, None, None, code=ARG, text="level out of range")
    call(e, P, None, 8, 4, U, 4, counts, None, code=ARG, text="level out of range")  # before dst, and counts_out stays
    assert list(counts) == [9] * 256
    call(e, P, None, 8, 4, U, 3, counts, None, code=ARG, text=NULL_DST)
    assert list(counts) == [0] * 256
    call(e, P, ODD, 8, 4, U, 3, None, None, code=ALIGN, text=ODD_DST)
    call(e, None, None, 8, 4, U, 3, None, None, code=ARG, text="null key pointer")
    counts[5] = 3
    call(e, None, None, 0, 4, U, 3, counts, None, code=OK)                    # len == 0: zero counts, no dst asked for
    assert list(counts) == [0] * 256
    call(e, P, None, 1, 4, U, 3, None, None, code=ARG, text=NULL_DST)         # one key is still moved


def test_split_top_level_device(call):
    e = "rdst_hip_split_top_level_device"
    call(e, P, P, 8, 4, U, None, None, code=ARG, text="null counts pointer")
    call(e, P, None, 8, 4, U, None, None, code=ARG, text="null counts pointer")   # before dst
    call(e, P, None, 8, 4, U, P, None, code=ARG, text=NULL_DST)
    call(e, P, ODD, 8, 4, U, P, None, code=ALIGN, text=ODD_DST)
    call(e, ODD, None, 8, 4, U, None, None, code=ALIGN, text="key pointer not aligned")


def test_level_count_entries(call):
    counts = (ctypes.c_uint64 * (4 * 256))(*([9] * 1024))
    call("rdst_hip_all_level_counts", P, 8, 4, U, 4, None, None, code=ARG, text="null counts_out")
    call("rdst_hip_all_level_counts", None, 8, 4, U, 4, None, None, code=ARG, text="null key pointer")
    call("rdst_hip_all_level_counts", None, 0, 4, U, 4, counts, None, code=OK)
    assert list(counts) == [0] * 1024
    one = (ctypes.c_uint64 * 256)(*([9] * 256))
    flags = (ctypes.c_uint8 * 3)(5, 5, 5)
    f = [ctypes.cast(ctypes.byref(flags, i), ctypes.POINTER(ctypes.c_uint8)) for i in range(3)]
    call("rdst_hip_level_counts", P, 8, 4, U, 4, one, None, None, None, None, code=ARG, text="level out of range")
    call("rdst_hip_level_counts", P, 8, 4, U, 4, None, None, None, None, None, code=ARG, text="level out of range")
    call("rdst_hip_level_counts", P, 8, 4, U, 3, None, None, None, None, None, code=ARG, text="null counts")
    assert list(one) == [9] * 256
    call("rdst_hip_level_counts", None, 0, 4, U, 3, one, f[0], f[1], f[2], None, code=OK)
    assert list(one) == [0] * 256 and list(flags) == [1, 0, 0]


def test_sort_records_integer_field(call):
    e = "rdst_hip_sort_records"
    call(e, P, 100, 24, 4, 3, U, None, code=UNSUPPORTED, text="record sorts take a 4- or 8-byte key field")
    call(e, P, 100, 24, 30, 3, U, None, code=UNSUPPORTED, text="4- or 8-byte key field")   # the width before the field's place
    call(e, P, 100, 24, 4, 4, 7, None, code=ARG, text="unknown key kind")
    call(e, P, 100, 24, 30, 4, 7, None, code=ARG, text="unknown key kind")                 # the kind before the field's place
    call(e, P, 100, 24, 24, 4, U, None, code=ARG, text="key field outside the record")
    call(e, P, 100, 24, 20, 8, S, None, code=ARG, text="key field outside the record")
    call(e, P, 100, 0, 0, 4, U, None, code=ARG, text="key field outside the record")
    call(e, P, 100, 24, 22, 4, U, None, code=ARG, text="key field outside the record")     # outside before misaligned
    call(e, P, 100, 24, 2, 4, U, None, code=ALIGN, text="key field not naturally aligned inside the record")
    call(e, P, 100, 22, 4, 4, U, None, code=ALIGN, text="not naturally aligned")           # the record size counts too
    call(e, P, 100, 24, 4, 8, F, None, code=ALIGN, text="not naturally aligned")
    call(e, None, 100, 24, 2, 4, U, None, code=ALIGN, text="not naturally aligned")        # misaligned before null
    call(e, None, 100, 24, 4, 4, U, None, code=ARG, text="null record pointer")
    call(e, None, 1 << 36, 24, 4, 4, U, None, code=ARG, text="null record pointer")        # null before the length
    call(e, P, 1 << 36, 24, 4, 4, U, None, code=ARG, text="len too large")
    call(e, P, 1, 24, 4, 4, U, None, code=OK)
    call(e, None, 0, 24, 4, 4, U, None, code=OK)
    call(e, P, 1, 24, 2, 4, U, None, code=ALIGN, text="not naturally aligned")             # checked for every length


def test_sort_records_bytes_field(call):
    e = "rdst_hip_sort_records"
    call(e, P, 100, 24, 4, 0, BYTES_BE, None, code=UNSUPPORTED, text="[u8; N] key fields are built for N in 1..RDST_BYTES_MAX_N")
    call(e, P, 100, 8192, 4, MAX_N + 1, BYTES_BE, None, code=UNSUPPORTED, text="[u8; N] key fields")
    call(e, P, 100, 24, 30, 0, BYTES_BE, None, code=UNSUPPORTED, text="[u8; N] key fields")   # the width before the field's place
    call(e, P, 100, 24, 22, 3, BYTES_BE, None, code=ARG, text="key field outside the record")
    call(e, P, 100, 0, 0, 3, BYTES_BE, None, code=ARG, text="key field outside the record")
    call(e, None, 100, 24, 22, 3, BYTES_BE, None, code=ARG, text="key field outside the record")  # outside before null
    call(e, None, 100, 24, 3, 5, BYTES_BE, None, code=ARG, text="null record pointer")
    call(e, None, 1 << 32, 24, 3, 5, BYTES_BE, None, code=ARG, text="null record pointer")    # null before the length
    call(e, P, 1 << 32, 24, 3, 5, BYTES_BE, None, code=UNSUPPORTED, text="records with a [u8; N] key are built for len < 2^32")
    call(e, P, 1, 24, 3, 5, BYTES_BE, None, code=OK)                  # any offset, any row size: no alignment rule here
    call(e, P, 1, 23, 3, 4, BYTES_BE, None, code=OK)
    call(e, None, 0, 24, 3, 5, BYTES_BE, None, code=OK)


def test_sort_bytes_keys_through_the_host_entry(call):
    e = "rdst_hip_sort"
    call(e, P, 100, 0, BYTES_BE, 0, None, code=UNSUPPORTED, text="[u8; N] keys are built for N in 1..RDST_BYTES_MAX_N")
    call(e, P, 100, MAX_N + 1, BYTES_BE, MAX_N + 1, None, code=UNSUPPORTED, text="[u8; N] keys are built for N in 1..RDST_BYTES_MAX_N")
    call(e, P, 100, 0, BYTES_BE, 3, None, code=UNSUPPORTED, text="[u8; N] keys are built")    # N before levels
    call(e, P, 100, 12, BYTES_BE, 11, None, code=ARG, text="levels must equal N for [u8; N]")
    call(e, P, 100, 12, BYTES_BE, 0, None, code=ARG, text="levels must equal N for [u8; N]")
    call(e, None, 100, 12, BYTES_BE, 11, None, code=ARG, text="levels must equal N")          # levels before null
    call(e, None, 100, 12, BYTES_BE, 12, None, code=ARG, text="null key pointer")
    call(e, None, 1 << 36, 12, BYTES_BE, 12, None, code=ARG, text="null key pointer")         # null before the length
    call(e, P, 1 << 36, 12, BYTES_BE, 12, None, code=ARG, text="len too large")
    call(e, P, 1 << 36, 40, BYTES_BE, 40, None, code=ARG, text="len too large")               # ... before the N > 16 limit
    call(e, P, 1 << 32, 17, BYTES_BE, 17, None, code=UNSUPPORTED, text="[u8; N] keys with N > 16 are built for len < 2^32")
    call(e, P, 1 << 32, MAX_N, BYTES_BE, MAX_N, None, code=UNSUPPORTED, text="N > 16 are built for len < 2^32")
    call(e, ODD + 1, 1, 12, BYTES_BE, 12, None, code=OK)              # rows have no alignment rule
    call(e, P, 1, 40, BYTES_BE, 40, None, code=OK)
    call(e, None, 0, 40, BYTES_BE, 40, None, code=OK)
