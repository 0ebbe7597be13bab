"""CPU-side checks of the rollup's share of the drop-in boundary (include/sybilgpu.h "rollup"): the two entry points are
exported and bound, the ctypes mirrors have the C compiler's sizes and offsets, NULL arguments are errors that leave *out NULL,
and tools/example_rollup.c links against the library as C99."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_bound_and_the_version_stays():
    from sybil_amd import _native as N
    lib = N.lib()
    for name in ("sybl_table_rollup", "sybl_table_rollup_stats"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.sybl_abi_version() == 6
    from sybil_amd.engine import Table
    assert callable(Table.rollup) and callable(Table.rollup_stats)


def test_mirrors_match_the_header(tmp_path):
    from sybil_amd import _native as N
    structs = {"sybl_rollup_agg": N.RollupAgg, "sybl_rollup_desc": N.RollupDesc, "sybl_rollup_stats": N.RollupStats}
    lines = []
    for cname, mirror in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in mirror._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sybilgpu.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).strip().split("\n"))
    want = {}
    for cname, mirror in structs.items():
        want[cname] = str(C.sizeof(mirror))
        for field, _ in mirror._fields_:
            want["%s.%s" % (cname, field)] = str(getattr(mirror, field).offset)
    assert got == want
    # every field the header declares is mirrored: the sizes leave no room for another
    assert C.sizeof(N.RollupStats) == 5 * 8 + 2 * 4 + 8 + 4 * 8 + 4 * 8 and C.sizeof(N.RollupAgg) == 16


def test_null_arguments_are_errors_and_leave_out_null():
    from sybil_amd import _native as N
    lib = N.lib()
    d = N.RollupDesc()
    h = C.c_void_p(0x1234)
    assert lib.sybl_table_rollup(None, C.byref(d), C.byref(h)) == N.E_INVAL
    assert h.value is None
    assert lib.sybl_last_error().decode().startswith("sybl_table_rollup: ")
    assert lib.sybl_table_rollup(None, None, None) == N.E_INVAL
    st = N.RollupStats()
    assert lib.sybl_table_rollup_stats(None, C.byref(st)) == N.E_INVAL
    assert lib.sybl_last_error().decode().startswith("sybl_table_rollup_stats: ")


def test_c_example_links_against_the_library(tmp_path):
    import sybil_amd
    libdir = os.path.dirname(os.path.abspath(sybil_amd.__file__))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_rollup.c"), "-L", libdir, "-lsybilgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "example_rollup")])
