"""Holds the restatement of table compute (tests/compute_ref.py) to answers written out by hand -- no GPU, no library."""
import numpy as np
import pytest

from tests import compute_ref as R

I64_MIN, I64_MAX = R.I64_MIN, R.I64_MAX
UNPOP = "unpopulated"

# (expression, expected): the arithmetic, precedence and populated-bit cases of the contract
KNOWN = [
    ("7 / -2", -3), ("-7 / 2", -3), ("-7 % 2", -1), ("7 % -2", 1), ("2 - 3 - 4", -5), ("100 / 10 / 5", 2),
    ("1 + 2 * 3 == 7 && !0", 1), ("1 < 2 == 1", 1), ("- - 3", 3), ("9223372036854775807 + 1", I64_MIN),
    ("-9223372036854775808 / -1", I64_MIN), ("-9223372036854775808 % -1", 0), ("abs(-9223372036854775808)", I64_MIN),
    ("3037000500 * 3037000500", -9223372036709301616), ("1 / 0", UNPOP), ("if(0, 1/0, 5)", 5), ("if(1/0, 1, 2)", UNPOP),
    ("coalesce(1/0, 9)", 9), ("0 && 1/0", UNPOP),
    # beyond the issue's table
    ("1 % 0", UNPOP), ("if(1, 1/0, 5)", UNPOP), ("1 || 1/0", UNPOP), ("coalesce(1/0, 2/0)", UNPOP), ("coalesce(3, 1/0)", 3),
    ("min(3, -4) + max(3, -4)", -1), ("!5 + !0", 1), ("2 * 3 % 4", 2), ("-2 * -3", 6), ("1 - -1", 2), ("(1 + 2) * 3", 9),
    ("1 <= 1 != 2 > 3", 1), ("0 || 0 && 1", 0), ("1 || 0 && 0", 1), ("-9223372036854775808", I64_MIN), ("9223372036854775808", I64_MIN),
    ("-9223372036854775807 - 2", I64_MAX), ("abs(-5) - abs(5)", 0), ("5 >= 5 == (4 < 5)", 1),
]


def _one(expr, types=None, cols=None):
    v, p = R.evaluate(expr, types or {}, cols or {}, 1)
    return v[0] if p[0] else UNPOP


@pytest.mark.parametrize("expr,want", KNOWN)
def test_known_answers(expr, want):
    assert _one(expr) == want


def test_has_names_and_functions_named_like_columns():
    types = {"x": "int", "a.b": "int", "min": "int", "s": "str", "tags": "set"}
    cols = {"x": ([77], [False]), "a.b": ([41], [True]), "min": ([10], [True]), "s": ([0], [True]), "tags": ([0], [False])}
    assert _one("has(x)", types, cols) == 0                       # 0, and populated
    assert _one("x + 1", types, cols) == UNPOP
    assert _one("coalesce(x, 0 - 1)", types, cols) == -1
    assert _one("`a.b` + 1", types, cols) == 42
    assert _one("min + min(min, 1)", types, cols) == 11           # the column and the function
    assert _one("has(s) + has(tags) * 2 + has(`a.b`) * 4", types, cols) == 5
    for bad in ("s + 1", "tags", "nope", "has(1)", "has()", "has(x, x)", "has(x + 1)", "min(1)", "min(1, 2, 3)", "abs()", "if(1, 2)", "foo(1)",
                "1 +", "(1", "1)", "", "1 2", "9223372036854775809", "1 & 2", "1 | 2", "1 = 2", "`x", "``", "2x", "1 << 2", "~1", "1.5"):
        with pytest.raises(R.ComputeError):
            R.compile_expr(bad, types)


def test_program_text_and_limits():
    t = {c: "int" for c in "abcdefghi"}
    assert R.text(R.compile_expr("a - b / 1000", t)[0]) == "c0 c1 1000 div sub"
    assert R.text(R.compile_expr("(a - b) / 1000", t)[0]) == "c0 c1 sub 1000 div"
    assert R.text(R.compile_expr("-a * !b", t)[0]) == "c0 neg c1 not mul"
    assert R.text(R.compile_expr("a < b == b >= a && a || has(b)", t)[0]) == "c0 c1 lt c1 c0 ge eq c0 and has(c1) or"
    assert R.text(R.compile_expr("if(a, min(a, b), coalesce(b, 1))", t)[0]) == "c0 c0 c1 min c1 1 coalesce if"
    assert R.compile_expr("a+b+c+d+e+f+g+h", t)[1] == list("abcdefgh")
    with pytest.raises(R.ComputeError, match="8 distinct"):
        R.compile_expr("a+b+c+d+e+f+g+h+i", t)
    ok = "+".join(["1"] * 32) + "+a"                                # 33 operands + 32 adds = 65 ops
    assert len(R.compile_expr("+".join(["1"] * 32) + "", t)[0]) == 63
    assert len(R.compile_expr("-(" + "+".join(["1"] * 32) + ")", t)[0]) == 64
    with pytest.raises(R.ComputeError, match="64 ops"):
        R.compile_expr(ok, t)
    deep8 = "1+(1+(1+(1+(1+(1+(1+(1" + ")" * 7
    assert R.compile_expr(deep8, t)[2] == 8
    with pytest.raises(R.ComputeError, match="stack"):
        R.compile_expr("1+(" + deep8 + ")", t)
    assert R.compile_expr("(" * 64 + "1" + ")" * 64, t)[2] == 1
    with pytest.raises(R.ComputeError, match="nested"):
        R.compile_expr("(" * 65 + "1" + ")" * 65, t)
    with pytest.raises(R.ComputeError):
        R.compile_expr("-" * 10000 + "1", t)


def test_compute_ref_storage_bitmap_and_chaining():
    b0 = (3, {"a": ("int", np.array([10, 20, 30]), None), "b": ("int", np.array([1, 0, 3]), np.array([True, True, False])), "s": ("str", ["x", None, "y"])})
    b1 = (0, {"a": ("int", np.zeros(0, dtype=np.int64), None)})
    b2 = (2, {"a": ("int", np.array([I64_MAX, -5]), None)})          # b and s absent: unpopulated for the block
    ref = R.compute_ref([b0, b1, b2], [("q", "a / b"), ("w", "a + 1"), ("z", "coalesce(q, has(s)) + w * 0"), ("none", "a / 0")], compact=True)
    assert ref["stats"] == {"rows": 5, "blocks": 2, "exprs": 4, "ops": 3 + 3 + 7 + 3, "unpopulated": 4 + 0 + 0 + 5}
    cols = R.D.concat(ref["blocks"])
    assert cols["q"][1].tolist() == [10, 0, 0, 0, 0] and cols["q"][2].tolist() == [True, False, False, False, False]
    assert cols["w"][1].tolist() == [11, 21, 31, I64_MIN, -4]
    assert cols["z"][1].tolist() == [10, 0, 1, 0, 0] and cols["z"][2].all()
    assert ref["storage"] == {"q": (1, 10), "w": (8, 0), "z": (1, 0), "none": (1, 0)}
    assert ref["has_missing"] == {"q": True, "w": False, "z": False, "none": True}
    assert ref["extrema"] == {"q": (10, 10), "w": (I64_MIN, 31), "z": (0, 10), "none": (I64_MAX, I64_MIN)}
    assert R.compute_ref([b0], [("q", "a * 300")], compact=True)["storage"]["q"] == (2, 3000)
    assert R.compute_ref([b0], [("q", "a * 100000000")], compact=True)["storage"]["q"] == (4, 1000000000)
    assert R.compute_ref([b0], [("q", "a * 300")], compact=False)["storage"]["q"] == (8, 0)
    for bad in ([("a", "1")], [("q", "1"), ("q", "2")], [("", "1")], [], [("q", "q + 1")], [("q", "s")]):
        with pytest.raises(R.ComputeError):
            R.compute_ref([b0], bad)
