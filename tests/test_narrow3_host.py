"""The 3-byte layout of a narrow twin (sybil_amd/csrc/narrow3.h: pack3, unpack3) on the host -- no GPU.

tests/narrow3_host_main.cpp is a program of its own around the header, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python).  It checks unpack3(pack3(u)) == u for 0, 1,
2^24 - 1, 0x010203 and 0xFDFEFF in every one of the four row positions and for 1e6 seeded random quadruples, that the byte image
of pack3 equals a plain 3-bytes-per-row little-endian write, and that a column written quad by quad reads back row by row at byte
3 * i.  The kernels around the layout are covered by tests/test_gpu_narrow_twin.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack3_and_unpack3_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "narrow3_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tests", "narrow3_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:3] == ["edge values ok", "random quads ok", "whole column ok"], run.stdout
    assert run.stderr == "", run.stderr
