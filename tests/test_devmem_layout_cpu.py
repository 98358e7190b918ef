"""The carved device buffers (csrc/lt_layouts.h on csrc/lt_devmem.h's lt_carve) are pure size_t arithmetic: a small C++
program, tests/devmem_layout_check.cpp, is compiled with the host compiler -- no HIP header, no GPU -- and holds the offsets
and totals of the five buffers against the expressions the sites used to write out, at 0, 1, 63, 64, 65, 255, 256, 257
elements and at one count whose byte size passes 2^32."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_transfer_amd", "csrc")


def test_layouts_match_the_sites_arithmetic(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (g++, c++, clang++) on this machine"
    exe = str(tmp_path / "devmem_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                            os.path.join(ROOT, "tests", "devmem_layout_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, "the layout headers must compile without HIP:\n" + build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "layouts ok"
