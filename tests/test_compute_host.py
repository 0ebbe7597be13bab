"""The parser and the host evaluator of compute expressions (sybil_amd/csrc/compute_expr.h, compute_ops.h) on the host -- no GPU.

tests/compute_host_main.cpp is a program of its own around the two headers, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python).  It evaluates the known answers of the
contract, compiles every prefix and every one-byte deletion of a set of valid expressions, 1e5 seeded random strings over the
grammar's alphabet and 10 000 nested parentheses, minus signs and min( calls: each is refused or evaluated, without a report."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_and_evaluator_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "compute_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tests", "compute_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:4] == ["known answers ok", "prefixes and deletions ok", "random strings ok", "deep nesting ok"], run.stdout
    assert run.stderr == "", run.stderr
