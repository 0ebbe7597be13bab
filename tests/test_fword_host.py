"""The layout of a filter word (sybil_amd/csrc/fword.h: fword_layout, fword_pack, fword_field) on the host -- no GPU.

tests/fword_host_main.cpp is a program of its own around the header, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python).  For the field sets 10/10/10, 11/11/10
(which uses bit 31), 1/1 and 16/8/8 it checks that fword_field(fword_pack(offsets)) gives the offsets back for 0, 1 and all ones
in every field position and for 1e6 seeded random rows per set, that the word equals the plain sum of the shifted offsets with
nothing above the last field, and that a bit changed in one field changes exactly that bit of the word and no other field.  The
kernels around the layout are covered by tests/test_gpu_filter_word.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_and_field_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "fword_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tests", "fword_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:3] == ["bit lengths ok", "edge values ok", "random rows ok"], run.stdout
    assert run.stderr == "", run.stderr
