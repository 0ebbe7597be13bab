"""The exact multiply-shift quotient of the PROVED row bodies (sybil_amd/csrc/udiv_magic.h) on the host -- no GPU.

tools/micro/udiv_magic_check.cpp is a program of its own around the header, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python).  For each divisor it recomputes the
multiplier in 64 bits -- at most 2^31, so below 2^32 -- and checks the quotient of EVERY numerator below 2^24 against a counted
n / d: for 1, 2, 3, 7, 641, 999, 1000, 1001, 4095, 4096, 4097, 65535, 65536, 65537, 2^23 - 1, 2^23, 2^23 + 1, 2^24 - 2, 2^24 - 1
and 300 seeded random divisors of every bit length 1 .. 24.  The header's own static_asserts (the edges of d = 1, 2, 3, 2^23,
2^23 + 1, 2^24 - 1) are compiled with it.  The kernels around the quotient are covered by tests/test_gpu_valu_diet.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_numerator_below_2_24_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "udiv_magic_check")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tools", "micro", "udiv_magic_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == "ok divisors=319 numerators=16777216\n", run.stdout
    assert run.stderr == "", run.stderr
