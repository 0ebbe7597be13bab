"""CPU-side checks of the digest part of the C ABI (include/sybilgpu.h, "digest").  Table.digest itself needs a GPU:
tests/test_gpu_digest.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_digest_entry_points_are_exported_and_bound():
    from sybil_amd import _native as N
    lib = N.lib()
    for name in ("sybl_table_digest", "sybl_table_digest_stats"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert lib.sybl_abi_version() == 6   # additive: the version does not move
    import sybil_amd.engine as E
    assert callable(E.Table.digest)


def test_header_compiles_as_c99_and_the_stats_mirror_has_its_layout(tmp_path):
    from sybil_amd import _native as N
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "sybilgpu.h"
int main(void){
  int (*f)(sybl_table *, const char *, int32_t, sybl_table **) = sybl_table_digest; (void)f;
  printf("%zu %zu %zu\n", sizeof(sybl_digest_stats), offsetof(sybl_digest_stats, keys_ms), offsetof(sybl_digest_stats, gather_bytes));
  return 0; }
'''
    (tmp_path / "d.c").write_text(prog)
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "d.c"),
                           "-L", libdir, "-lsybilgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "d")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "d")]).split()]
    assert out == [ctypes.sizeof(N.DigestStats), N.DigestStats.keys_ms.offset, N.DigestStats.gather_bytes.offset]


def test_null_arguments_are_errors_not_crashes():
    from sybil_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.sybl_table_digest(None, b"time", 0, ctypes.byref(h)) == N.E_INVAL
    assert b"NULL" in lib.sybl_last_error()
    assert lib.sybl_table_digest_stats(None, None) == N.E_INVAL
