"""The first-writer geometry of the owner-computes push (csrc/owner_geom.hpp: fresh_range, bricks_over) without a GPU:
tests/native/first_writer_geom.cpp rebuilds the ownership of every lattice point by brute force -- the boxes of the interior bricks in
the order of the colour launches -- for every folding and non-folding dim of n = 32 .. 120 and orders 1 - 3, and in 3-D on one small
lattice, and compares it with the functions.  A stand-alone host program, built here with AddressSanitizer and
UndefinedBehaviorSanitizer (it indexes the ownership maps with what the geometry functions return) and run once."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_writer_geometry(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the geometry check needs a host C++ compiler"
    exe = str(tmp_path / "first_writer_geom")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "torch-interpol_amd", "csrc"),
                            os.path.join(ROOT, "tests", "native", "first_writer_geom.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    assert run.stdout.startswith("ok ") and "runtime error" not in run.stdout, run.stdout
