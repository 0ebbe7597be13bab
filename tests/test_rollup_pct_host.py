"""The host plan of the rollup's percentiles (sybil_amd/csrc/rollup_plan.h: cbits, vbits, the sort variant, the forced
variants, the p<k> tokens, the rank) -- no GPU.

tests/rollup_pct_host_main.cpp is a program of its own around the header, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process, exactly as tests/test_rollup_host.py does (nothing is loaded into
python).  It checks vbits at spans 0, 1, 2^32 - 1, 2^32, 2^63 and the whole int64 range from bases at both int64 edges; the
variant on both sides of 32 and 64 total bits; cbits at 1 cell, 2 cells and 2^27 cells; the forced variants and their
refusals; the tokens; the rank without overflow.  The kernels around it are covered by tests/test_gpu_rollup_pct.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollup_pct_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "rollup_pct_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tests", "rollup_pct_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:5] == ["vbits ok", "cbits ok", "variants ok", "forced ok", "tokens ok"], run.stdout
    assert run.stderr == "", run.stderr
