"""CPU-side checks of the [u8; N] entry points for N beyond 16 (rdst_hip_sort_bytes_device, the widened rdst_hip_sort and
rdst_hip_sort_records): exported, sized, and every argument error returns before any device work."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_BE = 3
MAX_N = 4096


def test_new_symbols_are_exported(hiplib):
    from rdst_amd import _lib
    for name in ("rdst_hip_sort_bytes_device", "rdst_hip_sort_bytes_scratch_bytes"):
        assert name in _lib.SYMBOLS
        assert getattr(hiplib, name) is not None
    assert _lib.RDST_BYTES_MAX_N == MAX_N
    assert f"#define RDST_BYTES_MAX_N {MAX_N}u" in open(os.path.join(ROOT, "include", "rdst_hip.h")).read()


def test_scratch_size(hiplib):
    size = hiplib.rdst_hip_sort_bytes_scratch_bytes
    assert size(1000, 0) == 0
    assert size(1000, MAX_N + 1) == 0
    assert size(1000, 1) > 0 and size(1000, MAX_N) > 0
    for n_bytes in (1, 8, 16, 17, 20, 32, 64, 1000, MAX_N):
        for n in (2, 1000, 100_003, 10**8):
            assert size(n, n_bytes) >= n * n_bytes, (n, n_bytes)
        assert size(10**6, n_bytes) > size(10**3, n_bytes)
    widths = (1, 4, 8, 16, 17, 20, 24, 32, 64, 256, 1000, MAX_N)
    sizes = [size(10**6, nb) for nb in widths]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[4] > sizes[0]


def test_device_entry_argument_errors(hiplib):
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    scratch = (ctypes.c_uint8 * 8192)()
    sp = ctypes.c_void_p((ctypes.cast(scratch, ctypes.c_void_p).value + 255) // 256 * 256)
    f = hiplib.rdst_hip_sort_bytes_device
    assert f(p, 8, 0, sp, 4096, None) == -1                           # N = 0: LEVELS == 0
    assert f(p, 8, MAX_N + 1, sp, 4096, None) == -2                   # past the cap
    assert f(None, 8, 20, sp, 4096, None) == -1                       # null rows
    assert b"rows" in hiplib.rdst_hip_last_error()
    assert f(p, 1 << 32, 20, sp, 1 << 62, None) == -2                 # N > 16 needs len < 2^32
    assert f(p, 100, 20, None, 1 << 20, None) == -1                   # null scratch
    need = hiplib.rdst_hip_sort_bytes_scratch_bytes(100, 20)
    assert f(p, 100, 20, sp, need - 1, None) == -1                    # scratch too small
    assert b"scratch" in hiplib.rdst_hip_last_error()
    assert f(p, 10, 17, ctypes.c_void_p(sp.value + 1), 1 << 20, None) == -6  # scratch not 256-byte aligned
    # len <= 1 is a no-op (src/radix_sort_builder.rs:151), even without scratch
    assert f(p, 1, 20, None, 0, None) == 0
    assert f(p, 0, 4096, None, 0, None) == 0
    assert f(None, 0, 17, None, 0, None) == 0


def test_host_entry_argument_errors(hiplib):
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    before = bytes(buf)
    assert hiplib.rdst_hip_sort(p, 8, 20, BYTES_BE, 19, None) == -1         # levels != N
    assert b"levels" in hiplib.rdst_hip_last_error()
    assert hiplib.rdst_hip_sort(p, 8, MAX_N + 1, BYTES_BE, MAX_N + 1, None) == -2
    assert hiplib.rdst_hip_sort(None, 8, 20, BYTES_BE, 20, None) == -1
    assert hiplib.rdst_hip_sort(p, 1 << 32, 20, BYTES_BE, 20, None) == -2   # N > 16 needs len < 2^32
    assert hiplib.rdst_hip_sort(p, 1, 4096, BYTES_BE, 4096, None) == 0
    assert hiplib.rdst_hip_sort(p, 0, 20, BYTES_BE, 20, None) == 0
    assert bytes(buf) == before


def test_records_entry_argument_errors(hiplib):
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rec = hiplib.rdst_hip_sort_records
    assert rec(p, 8, 23, 3, 21, BYTES_BE, None) == -1                  # field past the row
    assert rec(p, 8, 23, 0, 0, BYTES_BE, None) == -2                   # N = 0
    assert rec(p, 8, 5000, 0, MAX_N + 1, BYTES_BE, None) == -2
    assert rec(None, 8, 23, 1, 20, BYTES_BE, None) == -1
    assert rec(p, 1 << 32, 23, 1, 20, BYTES_BE, None) == -2
    assert rec(p, 1, 23, 1, 20, BYTES_BE, None) == 0                   # len <= 1: no-op, any offset and stride
    assert rec(p, 0, 7, 3, 3, BYTES_BE, None) == 0
    # numeric key fields keep their rules
    assert rec(p, 8, 23, 1, 4, 0, None) == -6


def test_bytes_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_bytes.cpp")
    exe = str(tmp_path / "test_rdst_bytes")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)
