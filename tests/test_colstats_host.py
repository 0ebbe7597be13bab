"""The host rules of every column maker (sybil_amd/csrc/colstats.h: fit_storage, stats_fold, set_gather) -- no GPU.

tests/colstats_host_main.cpp is a program of its own around the header, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python).  It checks, against values written out
by hand or computed with __int128 / a plain loop in the program itself: the storage rule at canonical widths 4 and 8 for
ranges of 0, 255, 256, 65535, 65536, 2^32 - 1 and 2^32, for the whole int64 range, for a single value at INT64_MIN and for
nothing populated; the statistics fold with no block, with an empty block that carries INT64_MAX / INT64_MIN, behind existing
entries, at the int64 edges and with has_missing on and off; the set-column gather over a CSR of size 0 and 1, an all-none
map, a source row at off.size() - 1, repeated rows and a permutation.  The kernels around them are covered by
tests/test_gpu_digest.py, test_gpu_select.py, test_gpu_concat.py, test_gpu_lookup.py and test_gpu_compute.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_storage_rule_fold_and_set_gather_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "colstats_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tests", "colstats_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:3] == ["storage rule ok", "fold ok", "set gather ok"], run.stdout
    assert run.stderr == "", run.stderr
