"""CPU-side checks of the concat part of the C ABI (include/sybilgpu.h, "concat").  Context.concat itself needs a GPU:
tests/test_gpu_concat.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_concat_entry_points_are_exported_and_bound():
    from sybil_amd import _native as N
    lib = N.lib()
    for name in ("sybl_table_concat", "sybl_table_concat_stats"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert lib.sybl_abi_version() == 6   # additive: the version does not move
    import sybil_amd.engine as E
    assert callable(E.Context.concat) and callable(E.Table.concat_stats)


def test_header_compiles_as_c99_and_the_mirrors_have_their_layout(tmp_path):
    from sybil_amd import _native as N
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sybilgpu.h"
int main(void){
  int (*f)(const sybl_concat_desc *, sybl_table **) = sybl_table_concat; (void)f;
  int (*g)(const sybl_table *, sybl_concat_stats *) = sybl_table_concat_stats; (void)g;
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sybl_concat_desc), offsetof(sybl_concat_desc, tables), offsetof(sybl_concat_desc, n_columns),
         offsetof(sybl_concat_desc, columns), sizeof(sybl_concat_stats), offsetof(sybl_concat_stats, tables), offsetof(sybl_concat_stats, copies),
         offsetof(sybl_concat_stats, runs), offsetof(sybl_concat_stats, copy_ms), offsetof(sybl_concat_stats, copy_bytes));
  return 0; }
'''
    (tmp_path / "s.c").write_text(prog)
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "s")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert out == [ctypes.sizeof(N.ConcatDesc), N.ConcatDesc.tables.offset, N.ConcatDesc.n_columns.offset, N.ConcatDesc.columns.offset,
                   ctypes.sizeof(N.ConcatStats), N.ConcatStats.tables.offset, N.ConcatStats.copies.offset, N.ConcatStats.runs.offset,
                   N.ConcatStats.copy_ms.offset, N.ConcatStats.copy_bytes.offset]


def test_null_and_empty_arguments_are_errors_not_crashes():
    from sybil_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p(1)
    d = N.ConcatDesc()
    assert lib.sybl_table_concat(None, ctypes.byref(h)) == N.E_INVAL
    assert b"sybl_table_concat: " in lib.sybl_last_error() and h.value is None     # *out is NULL after a failure
    assert lib.sybl_table_concat(ctypes.byref(d), None) == N.E_INVAL
    assert lib.sybl_table_concat(None, None) == N.E_INVAL
    assert lib.sybl_table_concat(ctypes.byref(d), ctypes.byref(h)) == N.E_INVAL    # zero tables
    assert b"sybl_table_concat: " in lib.sybl_last_error()
    d.n_tables = 2
    assert lib.sybl_table_concat(ctypes.byref(d), ctypes.byref(h)) == N.E_INVAL    # a count without a list
    arr = (ctypes.c_void_p * 2)(None, None)
    d.tables = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
    assert lib.sybl_table_concat(ctypes.byref(d), ctypes.byref(h)) == N.E_INVAL    # a NULL entry
    assert b"sybl_table_concat: table 0 is NULL" in lib.sybl_last_error()
    assert lib.sybl_table_concat_stats(None, None) == N.E_INVAL
    assert b"sybl_table_concat_stats: NULL" in lib.sybl_last_error()
    st = N.ConcatStats()
    assert lib.sybl_table_concat_stats(None, ctypes.byref(st)) == N.E_INVAL


def test_c_concat_example_links_against_the_library(tmp_path):
    """tools/example_concat.c: two tables -> compact -> concat -> stats -> dictionary -> query -> free from C99, linked against
    the in-tree library."""
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_concat.c"), "-L", libdir, "-lsybilgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "example_concat")])
