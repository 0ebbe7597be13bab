"""CPU-side checks of the lookup part of the C ABI (include/sybilgpu.h, "lookup").  Table.lookup itself needs a GPU:
tests/test_gpu_lookup.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lookup_entry_points_are_exported_and_bound():
    from sybil_amd import _native as N
    lib = N.lib()
    for name in ("sybl_table_lookup", "sybl_table_lookup_stats"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert lib.sybl_abi_version() == 6   # additive: the version does not move
    import sybil_amd.engine as E
    assert callable(E.Table.lookup) and callable(E.Table.lookup_stats)


def test_header_compiles_as_c99_and_the_mirrors_have_their_layout(tmp_path):
    from sybil_amd import _native as N
    dfields = [f for f, _ in N.LookupDesc._fields_]
    sfields = [f for f, _ in N.LookupStats._fields_]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sybilgpu.h"
int main(void){
  int (*f)(sybl_table *, const sybl_lookup_desc *, sybl_table **) = sybl_table_lookup; (void)f;
  int (*g)(const sybl_table *, sybl_lookup_stats *) = sybl_table_lookup_stats; (void)g;
  printf("%zu %zu", sizeof(sybl_lookup_desc), sizeof(sybl_lookup_stats));
''' + "".join('  printf(" %%zu", offsetof(sybl_lookup_desc, %s));\n' % f for f in dfields) \
        + "".join('  printf(" %%zu", offsetof(sybl_lookup_stats, %s));\n' % f for f in sfields) + '  printf("\\n");\n  return 0; }\n'
    (tmp_path / "s.c").write_text(prog)
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "s")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert len(dfields) == 6 and len(sfields) == 15
    assert out == [ctypes.sizeof(N.LookupDesc), ctypes.sizeof(N.LookupStats)] \
        + [getattr(N.LookupDesc, f).offset for f in dfields] + [getattr(N.LookupStats, f).offset for f in sfields]


def test_null_arguments_are_errors_not_crashes():
    from sybil_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p(1234)
    d = N.LookupDesc()
    assert lib.sybl_table_lookup(None, ctypes.byref(d), ctypes.byref(h)) == N.E_INVAL
    assert lib.sybl_last_error().startswith(b"sybl_table_lookup: NULL")
    assert h.value is None                                   # *out is NULL after a failure
    assert lib.sybl_table_lookup(None, None, None) == N.E_INVAL
    assert lib.sybl_table_lookup(None, None, ctypes.byref(h)) == N.E_INVAL
    assert lib.sybl_table_lookup_stats(None, None) == N.E_INVAL
    assert lib.sybl_last_error().startswith(b"sybl_table_lookup_stats: NULL")
    st = N.LookupStats()
    assert lib.sybl_table_lookup_stats(None, ctypes.byref(st)) == N.E_INVAL


def test_c_lookup_example_links_against_the_library(tmp_path):
    """tools/example_lookup.c: two tables -> lookup -> stats -> a query grouped by an attached column -> free from C99, linked
    against the in-tree library."""
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_lookup.c"), "-L", libdir, "-lsybilgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "example_lookup")])
