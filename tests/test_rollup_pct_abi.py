"""CPU-side checks of the rollup percentiles' share of the drop-in boundary (include/sybilgpu.h "rollup"): the new entry
point is exported and bound, the ctypes mirror has the C compiler's size and offsets (80 bytes), NULL arguments are errors,
and the ABI version has not moved."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_bound_and_the_version_stays():
    from sybil_amd import _native as N
    lib = N.lib()
    assert hasattr(lib, "sybl_table_rollup_pct_stats") and "sybl_table_rollup_pct_stats" in N.SIGNATURES
    assert lib.sybl_abi_version() == 6
    from sybil_amd.engine import Table
    assert callable(Table.rollup_pct_stats)


def test_mirror_matches_the_header(tmp_path):
    from sybil_amd import _native as N
    cname, mirror = "sybl_rollup_pct_stats", N.RollupPctStats
    lines = ['printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for field, _ in mirror._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sybilgpu.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).strip().split("\n"))
    want = {cname: str(C.sizeof(mirror))}
    for field, _ in mirror._fields_:
        want["%s.%s" % (cname, field)] = str(getattr(mirror, field).offset)
    assert got == want
    assert [f for f, _ in mirror._fields_] == ["columns", "percentiles", "variant32", "variant64", "variant_pairs", "key_bits_max", "items",
                                               "keys_ms", "sort_ms", "pick_ms", "keys_bytes", "sort_bytes", "pick_bytes"]
    # every field the header declares is mirrored: the size leaves no room for another
    assert C.sizeof(mirror) == 6 * 4 + 8 + 3 * 8 + 3 * 8 == 80
    # the structs the rollup already had are as they were
    assert C.sizeof(N.RollupStats) == 5 * 8 + 2 * 4 + 8 + 4 * 8 + 4 * 8 and C.sizeof(N.RollupAgg) == 16


def test_null_arguments_are_errors():
    from sybil_amd import _native as N
    lib = N.lib()
    st = N.RollupPctStats()
    assert lib.sybl_table_rollup_pct_stats(None, C.byref(st)) == N.E_INVAL
    assert lib.sybl_last_error().decode().startswith("sybl_table_rollup_pct_stats: ")
    assert lib.sybl_table_rollup_pct_stats(None, None) == N.E_INVAL
    assert lib.sybl_last_error().decode().startswith("sybl_table_rollup_pct_stats: ")
