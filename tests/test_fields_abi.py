"""CPU-side checks of the described-key records route (rdst_key_field tables: rdst_hip_sort_records_by_fields, its device
form and its scratch size): exported, declared, sized, every argument error returns its code and a message before any device
work and leaves the caller's buffer as it was, and the Python mirror derives the right field table from a structured dtype."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
ARG, UNSUPPORTED, ALIGN = -1, -2, -6
MAX_N = 4096
NEW = ("rdst_hip_sort_records_by_fields", "rdst_hip_sort_records_by_fields_device", "rdst_hip_sort_records_by_fields_scratch_bytes")


def _table(fields):
    from rdst_amd import _lib
    return (_lib.KeyFieldC * max(1, len(fields)))(*[_lib.KeyFieldC(*f) for f in fields]), len(fields)


# (description, record_bytes, expected status): every argument error of the description
BAD = [
    ("no fields", [], 16, ARG),
    ("17 fields", [(i % 16, 1, UNSIGNED, 0) for i in range(17)], 16, UNSUPPORTED),
    ("L past the cap", [(0, 4096, BYTES_BE, 0), (0, 1, UNSIGNED, 0)], 4096, UNSUPPORTED),
    ("u24", [(0, 3, UNSIGNED, 0)], 16, UNSUPPORTED),
    ("i0", [(0, 0, SIGNED, 0)], 16, UNSUPPORTED),
    ("i32 bytes", [(0, 32, SIGNED, 0)], 64, UNSUPPORTED),
    ("f16", [(0, 2, FLOAT, 0)], 16, UNSUPPORTED),
    ("f128", [(0, 16, FLOAT, 0)], 16, UNSUPPORTED),
    ("empty byte string", [(0, 0, BYTES_BE, 0)], 16, UNSUPPORTED),
    ("byte string past the cap", [(0, MAX_N + 1, BYTES_BE, 0)], 5000, UNSUPPORTED),
    ("unknown kind", [(0, 4, 4, 0)], 16, ARG),
    ("unknown flag", [(0, 4, UNSIGNED, 2)], 16, ARG),
    ("unknown flag beside a known one", [(0, 4, UNSIGNED, 3)], 16, ARG),
    ("field past the record", [(13, 4, UNSIGNED, 0)], 16, ARG),
    ("second field past the record", [(0, 4, UNSIGNED, 0), (16, 1, UNSIGNED, 0)], 16, ARG),
    ("offset overflow", [(0xFFFFFFFF, 8, UNSIGNED, 0)], 16, ARG),
]


def test_symbols_header_and_constants(hiplib):
    from rdst_amd import _lib
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert getattr(hiplib, name) is not None
    assert hiplib.rdst_hip_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    assert "#define RDST_FIELD_DESCENDING 1u" in header and "#define RDST_KEY_FIELDS_MAX   16u" in header
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header
    struct = header[header.index("typedef struct {\n    uint32_t offset;"):]
    struct = struct[:struct.index("rdst_key_field;")]
    assert [ln.split(";")[0].split()[-1] for ln in struct.splitlines()[1:5]] == ["offset", "bytes", "kind", "flags"]
    for name in NEW:
        assert name + "(" in header
    assert "src/radix_key.rs" in header and "examples/impl_radix_key.rs:32-56" in header
    assert (_lib.RDST_FIELD_DESCENDING, _lib.RDST_KEY_FIELDS_MAX) == (1, 16)
    assert ctypes.sizeof(_lib.KeyFieldC) == 16


@pytest.mark.parametrize("what,fields,rec_bytes,status", BAD, ids=[b[0] for b in BAD])
def test_argument_errors_leave_the_buffer_alone(hiplib, what, fields, rec_bytes, status):
    buf = np.random.default_rng(5).integers(0, 256, size=8 * 5000, dtype=np.uint8)
    before = buf.copy()
    p = ctypes.c_void_p(buf.ctypes.data)
    scratch = (ctypes.c_uint8 * 8192)()
    sp = ctypes.c_void_p((ctypes.cast(scratch, ctypes.c_void_p).value + 255) // 256 * 256)
    table, nf = _table(fields)
    # a message of this very call: the previous one is replaced
    assert hiplib.rdst_hip_sort_bytes_device(p, 8, 0, sp, 4096, None) == ARG
    stale = hiplib.rdst_hip_last_error()
    assert hiplib.rdst_hip_sort_records_by_fields(p, 8, rec_bytes, table, nf, None) == status, what
    msg = hiplib.rdst_hip_last_error()
    assert msg and msg != stale
    assert hiplib.rdst_hip_sort_records_by_fields_device(p, 8, rec_bytes, table, nf, sp, 1 << 40, None) == status, what
    assert hiplib.rdst_hip_last_error() == msg
    assert hiplib.rdst_hip_sort_records_by_fields_scratch_bytes(8, rec_bytes, table, nf) == 0, what
    # an invalid description is an error at every length, the no-op lengths included
    assert hiplib.rdst_hip_sort_records_by_fields(p, 1, rec_bytes, table, nf, None) == status
    assert np.array_equal(buf, before)


def test_null_table_and_other_argument_errors(hiplib):
    buf = np.arange(4096, dtype=np.uint8)
    before = buf.copy()
    p = ctypes.c_void_p(buf.ctypes.data)
    scratch = (ctypes.c_uint8 * 8192)()
    sp = ctypes.c_void_p((ctypes.cast(scratch, ctypes.c_void_p).value + 255) // 256 * 256)
    host, dev, size = (getattr(hiplib, n) for n in NEW)
    table, nf = _table([(1, 2, UNSIGNED, 0), (4, 8, SIGNED, 1)])
    assert host(p, 8, 16, None, 2, None) == ARG and b"table" in hiplib.rdst_hip_last_error()
    assert dev(p, 8, 16, None, 2, sp, 4096, None) == ARG
    assert size(8, 16, None, 2) == 0
    assert host(None, 8, 16, table, nf, None) == ARG and b"record" in hiplib.rdst_hip_last_error()
    assert dev(None, 8, 16, table, nf, sp, 4096, None) == ARG
    assert host(p, 1 << 32, 16, table, nf, None) == UNSUPPORTED and b"2^32" in hiplib.rdst_hip_last_error()
    assert dev(p, 1 << 32, 16, table, nf, sp, 1 << 62, None) == UNSUPPORTED
    assert dev(p, 100, 16, table, nf, None, 1 << 20, None) == ARG and b"scratch" in hiplib.rdst_hip_last_error()
    need = size(100, 16, table, nf)
    assert need > 0
    assert dev(p, 100, 16, table, nf, sp, need - 1, None) == ARG and b"scratch" in hiplib.rdst_hip_last_error()
    assert dev(p, 100, 16, table, nf, ctypes.c_void_p(sp.value + 16), 1 << 20, None) == ALIGN
    assert np.array_equal(buf, before)


def test_len_up_to_one_is_a_no_op_with_null_pointers(hiplib):
    host, dev, _size = (getattr(hiplib, n) for n in NEW)
    for fields in ([(3, 1, UNSIGNED, 0)], [(0, 2, UNSIGNED, 0), (2, 8, SIGNED, 0)], [(1, 20, BYTES_BE, 1), (0, 4, FLOAT, 0)]):
        table, nf = _table(fields)
        for n in (0, 1):
            assert host(None, n, 24, table, nf, None) == 0
            assert dev(None, n, 24, table, nf, None, 0, None) == 0


def test_scratch_size(hiplib):
    size = hiplib.rdst_hip_sort_records_by_fields_scratch_bytes

    def of(n, rec_bytes, L):
        """two fields when L allows: a one-byte field and a byte string"""
        fields = [(0, 1, UNSIGNED, 0), (1, L - 1, BYTES_BE, 0)] if L > 1 else [(0, 1, UNSIGNED, 0)]
        return size(n, rec_bytes, *_table(fields))

    widths = (1, 2, 4, 5, 8, 9, 16, 17, 24, 64)
    for rec_bytes in (64, 200):
        for L in widths:
            for n in (2, 1000, 100_003, 10**8):
                assert of(n, rec_bytes, L) >= n * rec_bytes, (n, rec_bytes, L)
            by_len = [of(n, rec_bytes, L) for n in (2, 3, 255, 256, 257, 4097, 100_003, 10**6, 10**8)]
            assert by_len == sorted(by_len) and by_len[-1] > by_len[0]
        for n in (2, 1000, 10**6):
            by_width = [of(n, rec_bytes, L) for L in widths]
            assert by_width == sorted(by_width), (n, rec_bytes)
        # the key arrays grow at 4|5 (u32 -> u64 keys) and 8|9 (the order core and the packed keys), the packed keys at 16|17
        for a, b in ((4, 5), (8, 9), (16, 17)):
            assert of(10**6, rec_bytes, a) < of(10**6, rec_bytes, b)
    # the same key from one field or several: the same size
    assert size(1000, 32, *_table([(0, 8, UNSIGNED, 0)])) == size(1000, 32, *_table([(0, 4, FLOAT, 0), (4, 4, SIGNED, 1)]))


class _Recorder:
    """stands in for the loaded library: records the one call sort_host_records makes"""

    def __init__(self):
        self.calls = []

    def rdst_hip_sort_records_by_fields(self, ptr, n, rec_bytes, table, nf, opts):
        self.calls.append(("fields", n, rec_bytes, [(table[i].offset, table[i].bytes, table[i].kind, table[i].flags) for i in range(nf)]))
        return 0

    def rdst_hip_sort_records(self, ptr, n, rec_bytes, offset, nbytes, kind, opts):
        self.calls.append(("one", n, rec_bytes, offset, nbytes, kind))
        return 0


def test_python_maps_a_structured_dtype_to_the_field_table(monkeypatch):
    import rdst_amd
    from rdst_amd import _lib
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    packed = np.dtype({"names": ["tag", "tenant", "ts", "score", "id", "w", "pad"],
                       "formats": ["u1", "<u2", "<i8", "<f4", ("u1", (20,)), "<f8", "V3"],
                       "offsets": [0, 1, 3, 11, 15, 35, 43], "itemsize": 46})
    arr = np.zeros(10, dtype=packed)
    rdst_amd.sort_host_records(arr, ["tenant", "ts"])
    rdst_amd.sort_host_records(arr, [("score", "desc"), "id", ("tag", "asc"), ("w", "desc"), "pad"])
    rdst_amd.sort_host_records(arr, ("tenant",))
    rdst_amd.sort_host_records(arr, [rdst_amd.KeyField(3, 1, "unsigned"), rdst_amd.KeyField(1, 1, UNSIGNED, descending=True)])
    assert rec.calls == [
        ("fields", 10, 46, [(1, 2, UNSIGNED, 0), (3, 8, SIGNED, 0)]),
        ("fields", 10, 46, [(11, 4, FLOAT, 1), (15, 20, BYTES_BE, 0), (0, 1, UNSIGNED, 0), (35, 8, FLOAT, 1), (43, 3, BYTES_BE, 0)]),
        ("fields", 10, 46, [(1, 2, UNSIGNED, 0)]),
        ("fields", 10, 46, [(3, 1, UNSIGNED, 0), (1, 1, UNSIGNED, 1)]),
    ]
    # a plain str keeps taking the single-field entry
    aligned = np.zeros(10, dtype=[("k", "<f4"), ("v", "<u4")])
    rdst_amd.sort_host_records(aligned, "k")
    assert rec.calls[-1] == ("one", 10, 8, 0, 4, FLOAT)
    assert rdst_amd.key_fields_of(packed, [("ts", "desc")]) == [rdst_amd.KeyField(3, 8, "signed", True)]
    with pytest.raises(ValueError):
        rdst_amd.sort_host_records(arr, [("ts", "down")])
    with pytest.raises(TypeError):
        rdst_amd.sort_host_records(np.zeros(3, dtype=[("k", ">u4")]), ["k"])
    for name in ("KeyField", "key_fields_of", "sort_records_device_tensor"):
        assert name in rdst_amd.__all__


def test_fields_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_fields.cpp")
    exe = str(tmp_path / "test_rdst_fields")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)
