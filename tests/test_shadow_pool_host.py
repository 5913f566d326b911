"""How k_trace divides a launch's 64-ray groups among its waves (glaze_amd/csrc/device/trace_split.h), on the host, no GPU.

tests/shadow_pool_host.cpp includes the header the kernel includes and goes through grids of 1, 2, 7, 1 024 and 6 144 waves, closest-hit
groups and shadow rays from none to a few times the grid (ray counts that are no multiple of 64, below 64, zero), and every tuning value
of the sweep (static share 5 - 8 tenths, pool share 0, 1/8, 1/4, 1/2, chunks of 1, 2, 4 groups) plus a pool share of 1 and a chunk larger
than the pool: every shadow ray lies in exactly one shadow wave's static sequence or in exactly one pool chunk, 1 <= ws <= nw - 1, and
with the pool off the division is the formula k_trace had before, restated in the program."""
import os
import re
import shutil
import subprocess

from conftest import ROOT


def test_every_shadow_ray_has_one_place_and_pool_off_is_the_old_division(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host code: it must be there"
    exe = str(tmp_path / "shadow_pool_host")
    csrc = os.path.join(ROOT, "glaze_amd", "csrc")
    # the Makefile's host flags: the HIP headers give g++ empty __host__ / __device__
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "shadow_pool_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) inputs checked \((\d+) divide the waves\), 0 wrong\s*$", r.stdout)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) > 5000, r.stdout
