"""The host plan of a table rollup (sybil_amd/csrc/rollup_plan.h: radices, composite key, bucket range, path, slots) -- no GPU.

tests/rollup_host_main.cpp is a program of its own around the header, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python).  Against values written out by hand or
computed with __int128 in the program itself it checks: radices at ranges 0, 2^16 - 1, 2^16 and 2^61 from bases at the int64
edges, INT64_MIN / INT64_MAX as bounds and the whole int64 range; composites and strides, exactly 2^62 combinations accepted and
one more refused, no overflow of the running product; bucket ranges for negative lo and at the int64 edges; the path rule on
both sides of 2^16, 4 x rows, 2^27 and the 64 KiB LDS rule; slot sizing and its caps.  The kernels around it are covered by
tests/test_gpu_rollup.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollup_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "rollup_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tests", "rollup_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:5] == ["radices ok", "composites ok", "buckets ok", "paths ok", "slots ok"], run.stdout
    assert run.stderr == "", run.stderr
