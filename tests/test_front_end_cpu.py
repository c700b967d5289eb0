"""CPU test of the tile kernel's division pairs (csrc/jb_divmagic.h: what the launch computes once so that the kernel's
prologue divides by tiles_per_image, tiles_per_row and mcus_x with a multiply and a shift): tools/div_check.cpp, a
stand-alone program over the same header the host code and the kernels include, compares them with `/`."""
import os
import subprocess

from conftest import ROOT


def test_division_pairs_equal_the_division(tmp_path):
    exe = str(tmp_path / "div_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "jpeg_decoder_amd", "csrc"),
                        os.path.join(ROOT, "tools", "div_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    divisors, checked = map(int, r.stdout.split())
    assert divisors == 8192 + 3 * 18 + 1 and checked > 100 * divisors, r.stdout
