"""The piece table of k_scan_packed's dynamic dealing (sybil_amd/csrc/pieces.h: deal_pieces, piece_cap) on the host -- no GPU.

tests/pieces_host_main.cpp is a program of its own around the header, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python).  It deals single runs of 1, 4095, 4096,
4097 and 2^28 - 1, 2^28, 2^28 + 1 rows, many runs with gaps, and 200 random seeded run lists, at 1 .. 65536 tiles per piece, and
checks that every row of every run lies in exactly one piece, that the pieces are in table order, that none crosses a run's end
or a multiple of 2^28 rows from its run's start, that only a run's last piece is partial -- and that n_wg workgroups at their
caps have drawn at least n_pieces tickets.  The kernel around the table is covered by tests/test_gpu_dynamic_pieces.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deal_pieces_and_the_cap_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "pieces_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "sybil_amd", "csrc"), os.path.join(ROOT, "tests", "pieces_host_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split("\n")[:4] == ["single runs ok", "runs with gaps ok", "random runs ok", "cap ok"], run.stdout
    assert run.stderr == "", run.stderr
