"""include/rdst.hpp with keys described by a field table (rdst::sort_records_by): tests/cpp/test_rdst_fields.cpp on the device."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_rdst_fields.cpp")


def test_cpp_records_by_fields_match_std_stable_sort(tmp_path, gpu, hiplib):
    exe = str(tmp_path / "test_rdst_fields")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
