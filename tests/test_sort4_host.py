"""The node visit's child sort (glaze_amd/csrc/device/sort4.h: four keys in seven min / median / max operations) on the host, no GPU.

tests/sort4_host.cpp includes the header the tracers include -- the same sort4, with min3 / med3 / max3 written out where the device
names the instruction -- and holds it against std::sort for all 4^4 assignments of {three hit keys with different child bits, the miss
marker} to the four children, ascending (near first) and descending (far first, a pass of any-hit rays)."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_sort4_agrees_with_std_sort_on_every_assignment(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host code: it must be there"
    exe = str(tmp_path / "sort4_host")
    csrc = os.path.join(ROOT, "glaze_amd", "csrc")
    # the Makefile's host flags: the HIP headers give g++ empty __host__ / __device__
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "sort4_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("1024 assignments checked, 0 wrong")
