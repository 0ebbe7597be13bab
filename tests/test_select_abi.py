"""CPU-side checks of the select part of the C ABI (include/sybilgpu.h, "select").  Table.select itself needs a GPU:
tests/test_gpu_select.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_entry_points_are_exported_and_bound():
    from sybil_amd import _native as N
    lib = N.lib()
    for name in ("sybl_table_select", "sybl_table_select_stats"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert lib.sybl_abi_version() == 6   # additive: the version does not move
    import sybil_amd.engine as E
    assert callable(E.Table.select) and callable(E.Table.select_stats)


def test_header_compiles_as_c99_and_the_mirrors_have_their_layout(tmp_path):
    from sybil_amd import _native as N
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sybilgpu.h"
int main(void){
  int (*f)(sybl_table *, const sybl_select_desc *, sybl_table **) = sybl_table_select; (void)f;
  int (*g)(const sybl_table *, sybl_select_stats *) = sybl_table_select_stats; (void)g;
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(sybl_select_desc), offsetof(sybl_select_desc, columns), offsetof(sybl_select_desc, block_rows),
         sizeof(sybl_select_stats), offsetof(sybl_select_stats, filter_ms), offsetof(sybl_select_stats, gather_bytes));
  return 0; }
'''
    (tmp_path / "s.c").write_text(prog)
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "s")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert out == [ctypes.sizeof(N.SelectDesc), N.SelectDesc.columns.offset, N.SelectDesc.block_rows.offset,
                   ctypes.sizeof(N.SelectStats), N.SelectStats.filter_ms.offset, N.SelectStats.gather_bytes.offset]


def test_null_arguments_are_errors_not_crashes():
    from sybil_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p()
    d = N.SelectDesc()
    assert lib.sybl_table_select(None, ctypes.byref(d), ctypes.byref(h)) == N.E_INVAL
    assert b"sybl_table_select: NULL" in lib.sybl_last_error()
    assert lib.sybl_table_select(None, None, None) == N.E_INVAL
    assert lib.sybl_table_select_stats(None, None) == N.E_INVAL
    assert b"sybl_table_select_stats: NULL" in lib.sybl_last_error()
    st = N.SelectStats()
    assert lib.sybl_table_select_stats(None, ctypes.byref(st)) == N.E_INVAL


def test_c_select_example_links_against_the_library(tmp_path):
    """tools/example_select.c: create -> append -> select -> stats -> save -> free from C99, linked against the in-tree library."""
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_select.c"), "-L", libdir, "-lsybilgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "example_select")])
