"""The host-only half of the six rank entries (rdst_hip_topk_device, rdst_hip_select_device and their segmented forms):
rdst_args.h's address ranges, the scratch layouts of rdst_topk_layout.h and rdst_select_layout.h, the two check steps the
entries share and their size and limits functions (rdst_rank_args.cpp), as a stand-alone program under the sanitizers.  The
order of every whole entry is pinned through the built library by the *_abi.py files."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdst_amd", "csrc")


def test_host_half_under_sanitizers(tmp_path):
    """rdst_rank_args.cpp and rdst_segments.cpp with a main of their own, built with -fsanitize=address,undefined: a sanitizer
    report or a failed check is a non-zero exit.  Runs on the CPU as a child process; nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_rank_args_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_rank_args_host.cpp"), os.path.join(CSRC, "rdst_rank_args.cpp"),
           os.path.join(CSRC, "rdst_segments.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
