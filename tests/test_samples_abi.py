"""CPU-side checks of the samples part of the C ABI (include/sybilgpu.h, "samples"): the ctypes mirrors have the
compiler's struct sizes, and tools/example_samples.c builds against the in-tree library.  Table.samples itself needs a GPU
(sybil_amd.Context fails with -2 without one): tests/test_gpu_samples.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_samples_struct_layouts_match_header(tmp_path):
    from sybil_amd import _native as N
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sybilgpu.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu\n", sizeof(sybl_samples_desc), sizeof(sybl_samples_info), sizeof(sybl_samples_col),
  offsetof(sybl_samples_desc, limit), offsetof(sybl_samples_info, filter_ms), offsetof(sybl_samples_col, set_strings)); return 0; }
'''
    (tmp_path / "s.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"),
                           "-o", str(tmp_path / "s")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert out == [ctypes.sizeof(N.SamplesDesc), ctypes.sizeof(N.SamplesInfo), ctypes.sizeof(N.SamplesCol),
                   N.SamplesDesc.limit.offset, N.SamplesInfo.filter_ms.offset, N.SamplesCol.set_strings.offset]


def test_samples_entry_points_are_bound():
    from sybil_amd import _native as N
    lib = N.lib()
    for name in ("sybl_table_samples", "sybl_samples_free", "sybl_samples_get_info", "sybl_samples_column",
                 "sybl_samples_row_ids", "sybl_samples_render"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert lib.sybl_abi_version() == 6   # additive: the version does not move


def test_null_arguments_are_errors_not_crashes():
    from sybil_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.sybl_table_samples(None, None, ctypes.byref(h)) == N.E_INVAL
    assert b"NULL" in lib.sybl_last_error()
    assert lib.sybl_samples_get_info(None, None) == N.E_INVAL
    assert lib.sybl_samples_column(None, 0, None) == N.E_INVAL
    assert lib.sybl_samples_row_ids(None, None) == N.E_INVAL
    assert lib.sybl_samples_render(None) is None
    lib.sybl_samples_free(None)


def test_c_samples_example_links_against_the_library(tmp_path):
    """tools/example_samples.c: open -> samples -> columns -> render -> free from C99, linked against the in-tree library."""
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_samples.c"), "-L", libdir, "-lsybilgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "example_samples")])
