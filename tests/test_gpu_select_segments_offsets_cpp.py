"""include/rdst.hpp's mirrors of the segmented select with device-resident offsets (rdst::select_segments_device_offsets,
keys only and with an index): tests/cpp/test_rdst_select_segments_offsets.cpp on the device."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_rdst_select_segments_offsets.cpp")


def test_cpp_select_segments_device_offsets_matches_std_stable_sort(tmp_path, gpu, hiplib):
    exe = str(tmp_path / "test_rdst_select_segments_offsets")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
