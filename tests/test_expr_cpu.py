"""The expression layer without a GPU: one corpus of expressions -- the cases of test_strcmp_cpu, test_like_cpu, test_in_set_cpu,
test_scalar_functions_cpu and tests/golden/planner_cases.py plus the traps of the grammar -- and, for each, what columns_of,
compile_expr, result_type, the dictionary lowering over fake dictionaries, _choose_in_sets and lower_in_sets (over a fake probe)
make of it, with VNM_IN_SET_MIN at 1, 4 and 17 where a list is involved.

EXPECTED holds literals recorded by running record() below against commit 058be4a, the parent of the commit that introduced
vinum_amd.expr and core.lowering (there the lowering was FilterOperator.lower_dictionary_predicates): the expression layer is a
refactor, so it computes what that commit computed.  PARENT_DIFFERED lists the records that are NOT the parent's, with what the
parent gave:
  * a symbol-spelled comparison of a dictionary-coded column with a string literal now lowers as its named spelling does (the
    parent passed it through and compile_expr then raised KeyError: 'lit');
  * an empty IN list raises the ValueError written for it (the parent's desugaring walked into the empty value list first and
    raised IndexError: tuple index out of range);
  * columns_of no longer takes the NAME of an ("fn", name, ...) node for a column (the planner stripped such nodes first).
"""
import hashlib
import os
import subprocess
import sys

import pyarrow as pa
import pytest

from vinum_amd import expr as E
from vinum_amd import ops
from vinum_amd.core.base import DeviceRecordBatch
from vinum_amd.core.lowering import lower_dictionary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeDict:
    """what the lowerings ask of a KeyDictionary"""

    def __init__(self, name, arrow_type=pa.string(), on_device=True):
        self.name, self.type, self.on_device = name, arrow_type, on_device

    def translate_table(self, other):
        return f"<codes of {self.name} in {other.name}>"

    def joint_rank_tables(self, other):
        return f"<joint ranks of {self.name}>", f"<joint ranks of {other.name}>"

    def rank_column(self, col):
        return f"<ranks of {col.name}>"

    def like_table(self, pattern):
        return f"<like {pattern!r} in {self.name}>"

    def code_of(self, value):
        return {"Berlin": 3, b"Berlin": 3, "Paris": 5}.get(value)

    def rank_bounds(self, value):
        return 2, 1


class FakeColumn:
    vnm_type = 3          # L.I64
    length = 10

    def __init__(self, name, dictionary=None, arrow_type=pa.int64()):
        self.name, self.dictionary, self.arrow_type = name, dictionary, arrow_type


NUMERIC = ("v", "w", "k", "x", "y", "g", "i", "total", "tip", "fare", "lat", "n")


def _batch():
    """a, b: two dictionaries; s1, s2: one shared; s: its own; h: a host-route dictionary; NUMERIC: no dictionary"""
    shared = FakeDict("S")
    cols = {"a": FakeColumn("a", FakeDict("A")), "b": FakeColumn("b", FakeDict("B", pa.large_string())),
            "s1": FakeColumn("s1", shared), "s2": FakeColumn("s2", shared), "s": FakeColumn("s", FakeDict("SS")),
            "h": FakeColumn("h", FakeDict("H", pa.decimal128(10, 2), on_device=False))}
    cols.update({n: FakeColumn(n) for n in NUMERIC})
    return DeviceRecordBatch(cols, 0)


TYPES = {"v": (pa.int64(), False), "w": (pa.float64(), False), "k": (pa.int64(), False), "x": (pa.int64(), False),
         "y": (pa.int32(), True), "g": (pa.int8(), False), "i": (pa.int32(), False), "total": (pa.float64(), False),
         "tip": (pa.float64(), True), "fare": (pa.float32(), False), "lat": (pa.float64(), False), "n": (pa.int64(), True),
         "a": (pa.int32(), True), "b": (pa.int32(), False), "s": (pa.int32(), False), "h8": (pa.int8(), False)}
SYMBOLS = {"==": "eq", "=": "eq", "!=": "ne", "<>": "ne", "<": "lt", "<=": "le", ">": "gt", ">=": "ge"}


def _r(n, start=0):
    return tuple(range(start, start + n))


def _corpus():
    c = {}
    for op in ("eq", "ne", "lt", "le", "gt", "ge"):
        c[f"litcmp_{op}"] = (op, "a", ("lit", "Berlin"))
        c[f"litcmp_flipped_{op}"] = (op, ("lit", "Berlin"), "a")
    for op in ("eq", "lt", "ge"):
        c[f"colcol_{op}"] = (op, "a", "b")
    for sym in SYMBOLS:
        c[f"symlit_{sym}"] = (sym, "a", ("lit", "Berlin"))
        c[f"symlit_flipped_{sym}"] = (sym, ("lit", "Berlin"), "a")
    c.update({
        "symnum_eq": ("=", "v", 3), "symnum_ne": ("<>", "v", 3), "symnum_le": ("<=", "w", 2.5),
        "shared_eq": ("eq", "s1", "s2"), "shared_lt": ("lt", "s1", "s2"),
        "between_cols": ("between", "a", "b", "s1"), "not_between_cols": ("not_between", "a", "b", "b"),
        "nest": ("or", ("and", ("eq", "a", "b"), ("gt", "v", 3)), ("not", ("lt", "b", "a")), ("eq", "a", ("lit", "Berlin")),
                 ("to_int", ("ne", "a", "b"))),
        "litcmp_absent": ("eq", "a", ("lit", "Rome")), "litcmp_bytes": ("ne", "a", ("lit", b"Berlin")),
        "sym_colcol_eq": ("==", "a", "b"), "sym_colcol_lt": ("<", "a", "b"), "sym_numeric": (">", "v", "w"),
        "string_fn": ("upper", "a"), "other_fn": ("some_function", "h", ("eq", "a", "b")),
        "like": ("like", "a", ("lit", "Jos%")), "not_like": ("not_like", "s", ("lit", "")),
        "like_and": ("and", ("like", "s", ("lit", "a_c")), ("gt", "v", 3)), "like_not": ("not", ("like", "a", ("lit", "ü%"))),
        "like_to_int": ("to_int", ("like", "s", ("lit", "%b%"))),
        "like_twice": ("or", ("like", "a", ("lit", "x%")), ("not_like", "a", ("lit", "%y"))),
        "like_one_operand": ("like", "a"), "like_number_pattern": ("like", "a", ("lit", 5)),
        "like_column_pattern": ("like", "a", "b"), "like_numeric_column": ("like", "v", ("lit", "a%")),
        "like_unknown_column": ("like", "zz", ("lit", "a%")), "like_expression_operand": ("like", ("upper", "a"), ("lit", "a%")),
        "in_3": ("in", "k", (1, 2, 3)), "in_4": ("in", "k", (1, 2, 3, 4)), "in_16": ("in", "k", _r(16, 100)),
        "not_in_16": ("not_in", "k", _r(16, 100)), "in_17_and": ("and", ("in", "k", _r(17)), ("gt", "k", 3)),
        "not_in_17": ("not_in", "k", _r(17)), "in_two_tens": ("and", ("in", "x", _r(10)), ("in", "y", _r(11))),
        "in_three": ("and", ("in", "x", _r(10)), ("in", "y", _r(11)), ("in", "x", _r(12))),
        "in_mixed": ("or", ("in", "k", (1, 2)), ("not_in", "k", (3, 4, 5)), ("in", "k", (6,))),
        "in_1000": ("in", "k", _r(1000)), "in_1000_expr": ("to_int", ("not_in", ("add", "k", 1), _r(1000))),
        "in_f16_operand": ("in", ("sqrt", "h8"), _r(17)), "in_predicate_operand": ("in", ("gt", "k", 1), _r(17)),
        "in_floats": ("in", "w", (1, 2.5, 3)), "in_empty": ("in", "k", ()),
        "in_dict_strs": ("in", "a", ("Berlin", "Paris", "Rome")), "in_dict_lits": ("not_in", "a", (("lit", "Berlin"), ("lit", "Oslo"))),
        "in_dict_none_held": ("in", "a", ("Oslo",)), "in_dict_long": ("in", "a", ("Berlin", "Paris") * 10),
        "scalar_sqrt": ("sqrt", "total"), "scalar_to_int": ("to_int", ("mul", ("sin", "lat"), 100000)),
        "scalar_pi": ("add", "fare", ("pi",)), "scalar_abs": ("abs", ("sub", "total", "tip")), "scalar_power": ("power", "fare", 2),
        "scalar_to_float": ("to_float", "n"), "scalar_to_bool": ("to_bool", "n"), "scalar_e": ("mul", ("e",), ("cos", "lat")),
        "fold_sqrt": ("mul", ("sqrt", 4), "v"), "fold_nested": ("add", "v", ("to_int", ("log10", 1000.0))),
        "fold_negative_power": ("power", 2, -1), "power_negative_literal": ("power", "i", -2),
        "power_folded_exponent": ("add", 1, ("power", ("abs", "i"), ("to_int", -3.5))), "power_neg": ("power", "i", ("neg", 2)),
        "power_arity": ("power", "i"), "bool_literal": ("add", "v", True),
        "planner_between_in": ("and", ("between", "v", 10, 50.5), ("in", "k", (4, 11, 18, 410))),
        "planner_not_between_not_in": ("and", ("not_between", "i", -900, 900), ("not_in", "g", (0, 6))),
        "planner_is_null": ("is_null", "y"), "planner_is_not_null": ("and", ("is_not_null", "tip"), ("gt", "tip", 0.5)),
        "planner_arith": ("mul", ("sub", 1, "total"), ("add", 2, "tip")),
        "column": "v", "number": 7, "strong": ("add", "v", ("strong", 2.5)), "lookup": ("not", ("lookup", "s", "__t")),
        "lookup_i32": ("eq", "a", ("lookup_i32", "b", "__t")), "unknown_operator": ("frobnicate", "v"),
        "lit_alone": ("eq", "v", ("lit", "x")),
        # the traps: a value list whose members name columns, a literal that names one, a strong constant beside LIKE, BETWEEN over a
        # dictionary-coded operand, a list inside a list's operand, a function name
        "trap_value_list_names_columns": ("in", "k", ("a", "b")), "trap_literal_names_a_column": ("eq", "s", ("lit", "v")),
        "trap_strong_beside_like": ("and", ("like", "a", ("lit", "x%")), ("gt", "v", ("strong", 3))),
        "trap_between_dictionary_literals": ("between", "a", ("lit", "A"), ("lit", "M")),
        "trap_nested_in": ("in", ("to_int", ("in", "k", (1, 2, 3, 4, 5))), (0, 1)),
        "trap_fn": ("fn", "sum", ("add", "x", 1)),
    })
    return c


CORPUS = _corpus()
RECORDS = [(name, least) for name, e in CORPUS.items()
           for least in ((1, 4, 17) if "'in'" in repr(e) or "'not_in'" in repr(e) else (4,))]


def _plain(x):
    """a result as literals: long tuples and programs by length and digest, Arrow types by name"""
    if isinstance(x, (tuple, list)):
        if len(x) >= 40:
            return ("long", len(x), hashlib.sha1(repr(x).encode()).hexdigest()[:12])
        return tuple(_plain(y) for y in x)
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    return str(x) if isinstance(x, pa.DataType) else x


def _attempt(f):
    try:
        return _plain(f())
    except Exception as exc:  # noqa: BLE001 -- the class and the message are part of the record
        return ("raises", type(exc).__name__, str(exc))


def _program(e):
    names = ops.columns_of(e)
    return [(p.op, p.arg, p.imm_f, p.imm_i) for p in ops.compile_expr(e, {n: i for i, n in enumerate(names)})]


def _fake_probe(col, values, invert=False, length=None, stream=None):
    return f"<mask of {getattr(col, 'name', col)} over {len(tuple(values))}>"


def _fake_project_typed(e, columns, length=None, stream=None):
    return FakeColumn(f"<projected {e!r}>"[:60]), ops._result_type_code(e, {n: TYPES[n] for n in columns})


def record(name, least, setenv, setattr):
    """the dump of one expression with VNM_IN_SET_MIN = least"""
    setenv("VNM_IN_SET_MIN", str(least))
    setattr(ops, "in_set_probe", _fake_probe)
    setattr(ops, "_project_typed", _fake_project_typed)
    e = CORPUS[name]

    def in_sets():
        b = _batch()
        low, extra = lower_dictionary(e, b.columns)
        return ops.lower_in_sets(low, {**b.columns, **extra}, 10)
    return {"columns_of": _attempt(lambda: ops.columns_of(e)), "program": _attempt(lambda: _program(e)),
            "result_type": _attempt(lambda: ops.result_type(e, TYPES)),
            "lowered": _attempt(lambda: lower_dictionary(e, _batch().columns)),
            "chosen": _attempt(lambda: [(n[0], n[1], len(n[2])) for n in ops._choose_in_sets(e)]),
            "in_sets": _attempt(in_sets)}


@pytest.mark.parametrize("name,least", RECORDS)
def test_corpus_computes_what_the_parent_computed(name, least, monkeypatch):
    assert record(name, least, monkeypatch.setenv, monkeypatch.setattr) == EXPECTED[f"{name}@{least}"]


@pytest.mark.parametrize("sym,named", list(SYMBOLS.items()))
@pytest.mark.parametrize("flipped", [False, True])
def test_a_symbol_spelling_lowers_to_what_its_name_lowers_to(sym, named, flipped, monkeypatch):
    tail = "_flipped_" if flipped else "_"
    got = record(f"symlit{tail}{sym}", 4, monkeypatch.setenv, monkeypatch.setattr)
    want = EXPECTED[f"litcmp{tail}{named}@4"]
    assert got["lowered"] == want["lowered"] and got["in_sets"] == want["in_sets"] and got["lowered"][0][0] != "raises"
    assert got["lowered"][0][0] in E.CMP_FLIP                # a numeric compare the interpreter takes: no "lit" left
    assert "lit" not in repr(got["lowered"][0])


def test_parent_differed_only_where_listed():
    assert set(PARENT_DIFFERED) <= set(EXPECTED)
    for key, fields in PARENT_DIFFERED.items():
        assert all(EXPECTED[key][f] != was for f, was in fields.items()), key
    assert {k.split("@")[0] for k in PARENT_DIFFERED} == {f"symlit{t}{s}" for s in SYMBOLS for t in ("_", "_flipped_")} | {"in_empty", "trap_fn"}


def test_the_traps_hold():
    b = _batch()
    assert E.columns_of(("in", "k", ("a", "b"))) == ["k"]                      # a value list holds values, not columns
    assert lower_dictionary(("in", "k", ("a", "b")), b.columns) == (("in", "k", ("a", "b")), {})
    assert E.columns_of(("eq", "s", ("lit", "v"))) == ["s"]                    # "v" is a literal here, whatever the batch holds
    assert lower_dictionary(("eq", "s", ("lit", "v")), b.columns) == (("eq", "s", -2), {})
    strong = ("strong", 3)
    low, extra = lower_dictionary(("and", ("like", "a", ("lit", "x%")), ("gt", "v", strong)), b.columns)
    assert low == ("and", ("lookup", "a", "__like_0_a"), ("gt", "v", strong)) and low[2][2] is strong
    low, extra = lower_dictionary(("between", "a", ("lit", "A"), ("lit", "M")), b.columns)
    assert low == ("and", ("ge", "__rank_a", 2), ("lt", "__rank_a", 3)) and list(extra) == ["__rank_a"]
    inner = ("in", "k", (1, 2, 3, 4, 5))
    outer = ("in", ("to_int", inner), (0, 1))
    assert list(E.nodes(outer))[:3] == [outer, ("to_int", inner), inner] and E.columns_of(outer) == ["k"]
    assert E.operands(("fn", "sum", ("add", "x", 1))) == (("add", "x", 1),)    # the name is no operand
    assert E.columns_of(("fn", "sum", ("add", "x", 1))) == ["x"]
    for leaf in (("lit", "between"), ("strong", 2)):
        assert E.operands(leaf) == () and E.fold(leaf) is leaf and E.desugar(leaf) is leaf


def test_untouched_subtrees_keep_their_identity():
    vals = tuple(range(20))
    keep = ("in", ("add", "k", 1), vals)
    tree = ("and", keep, ("or", ("between", "v", 1, 2), ("fn", "sum", "x")), ("is_null", "y"))
    assert E.with_operands(keep, [keep[1]]) is keep and E.with_operands(tree, list(tree[1:])) is tree
    assert E.with_operands(keep, ["k"]) == ("in", "k", vals) and E.with_operands(keep, ["k"])[2] is vals
    assert E.with_operands(("fn", "sum", "x"), ["y"]) == ("fn", "sum", "y")
    with pytest.raises(ValueError, match="2 operand"):          # too few or too many: refused, never a truncated or a longer node
        E.with_operands(("add", "x", 1), ["x"])
    assert E.rewrite(tree, lambda n: None) is tree and E.transform(tree, lambda n: n) is tree
    got = E.rewrite(tree, lambda n: ("ge", "v", 1) if n[0] == "between" else None)
    assert got == ("and", keep, ("or", ("ge", "v", 1), ("fn", "sum", "x")), ("is_null", "y"))
    assert got[1] is keep and got[3] is tree[3] and got[2][2] is tree[2][2]
    seen = []
    E.rewrite(tree, lambda n: seen.append(n[0]) or (n if n[0] == "in" else None))
    assert seen == ["and", "in", "or", "between", "fn", "is_null"]              # top-down; a replaced subtree is finished
    seen = []
    E.transform(tree, lambda n: seen.append(n[0]) or n)
    assert seen == ["add", "in", "between", "fn", "or", "is_null", "and"]       # bottom-up


def test_one_comparison_table():
    assert E.CMP_SYMBOL == {"eq": "==", "ne": "!=", "gt": ">", "ge": ">=", "lt": "<", "le": "<="}
    assert E.CMP_FLIP == {"lt": "gt", "le": "ge", "gt": "lt", "ge": "le", "eq": "eq", "ne": "ne"}
    assert all(E.cmp_name(s) == n and E.cmp_name(n) == n for s, n in SYMBOLS.items()) and set(E.CMP_SYMBOLS) == set(SYMBOLS)
    assert E.cmp_name("and") is None and E.cmp_name("in") is None
    assert all(ops._EX[s] == ops._EX[n] for s, n in SYMBOLS.items()) and set(ops.CMP_OPS) == set(SYMBOLS)


def test_the_grammar_imports_without_the_library(tmp_path):
    """vinum_amd.expr in a fresh process, from a copy of the package that has no lib/"""
    pkg = tmp_path / "vinum_amd"
    pkg.mkdir()
    for f in ("__init__.py", "expr.py"):
        (pkg / f).write_bytes(open(os.path.join(ROOT, "vinum_amd", f), "rb").read())
    code = ("import sys; import vinum_amd.expr as E; "
            "assert 'vinum_amd._lib' not in sys.modules and 'vinum_amd.ops' not in sys.modules; "
            "print(E.columns_of(('in', ('add', 'a', 'b'), ('c',))))")
    out = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, capture_output=True, text=True, env={**os.environ, "PYTHONPATH": ""})
    assert out.returncode == 0 and out.stdout.strip() == "['a', 'b']", out.stderr


# what commit 058be4a gave where EXPECTED does not follow it (see the module docstring)
PARENT_DIFFERED = {
    'symlit_==@4': {
        'lowered': (('==', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('==', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_==@4': {
        'lowered': (('==', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('==', ('lit', 'Berlin'), 'a'), {}),
    },
    'symlit_=@4': {
        'lowered': (('=', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('=', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_=@4': {
        'lowered': (('=', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('=', ('lit', 'Berlin'), 'a'), {}),
    },
    'symlit_!=@4': {
        'lowered': (('!=', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('!=', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_!=@4': {
        'lowered': (('!=', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('!=', ('lit', 'Berlin'), 'a'), {}),
    },
    'symlit_<>@4': {
        'lowered': (('<>', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('<>', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_<>@4': {
        'lowered': (('<>', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('<>', ('lit', 'Berlin'), 'a'), {}),
    },
    'symlit_<@4': {
        'lowered': (('<', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('<', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_<@4': {
        'lowered': (('<', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('<', ('lit', 'Berlin'), 'a'), {}),
    },
    'symlit_<=@4': {
        'lowered': (('<=', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('<=', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_<=@4': {
        'lowered': (('<=', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('<=', ('lit', 'Berlin'), 'a'), {}),
    },
    'symlit_>@4': {
        'lowered': (('>', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('>', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_>@4': {
        'lowered': (('>', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('>', ('lit', 'Berlin'), 'a'), {}),
    },
    'symlit_>=@4': {
        'lowered': (('>=', 'a', ('lit', 'Berlin')), {}),
        'in_sets': (('>=', 'a', ('lit', 'Berlin')), {}),
    },
    'symlit_flipped_>=@4': {
        'lowered': (('>=', ('lit', 'Berlin'), 'a'), {}),
        'in_sets': (('>=', ('lit', 'Berlin'), 'a'), {}),
    },
    'in_empty@1': {
        'program': ('raises', 'IndexError', 'tuple index out of range'),
        'result_type': ('raises', 'IndexError', 'tuple index out of range'),
        'chosen': ('raises', 'IndexError', 'tuple index out of range'),
        'in_sets': ('raises', 'IndexError', 'tuple index out of range'),
    },
    'in_empty@4': {
        'program': ('raises', 'IndexError', 'tuple index out of range'),
        'result_type': ('raises', 'IndexError', 'tuple index out of range'),
        'chosen': ('raises', 'IndexError', 'tuple index out of range'),
        'in_sets': ('raises', 'IndexError', 'tuple index out of range'),
    },
    'in_empty@17': {
        'program': ('raises', 'IndexError', 'tuple index out of range'),
        'result_type': ('raises', 'IndexError', 'tuple index out of range'),
        'chosen': ('raises', 'IndexError', 'tuple index out of range'),
        'in_sets': ('raises', 'IndexError', 'tuple index out of range'),
    },
    'trap_fn@4': {
        'columns_of': ('sum', 'x'),
    },
}

EXPECTED = {
    'litcmp_eq@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('eq', 'a', 3), {}),
    },
    'litcmp_flipped_eq@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('eq', 'a', 3), {}),
    },
    'litcmp_ne@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ne', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('ne', 'a', 3), {}),
    },
    'litcmp_flipped_ne@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ne', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('ne', 'a', 3), {}),
    },
    'litcmp_lt@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 2), {}),
    },
    'litcmp_flipped_lt@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 3), {}),
    },
    'litcmp_le@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 3), {}),
    },
    'litcmp_flipped_le@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 2), {}),
    },
    'litcmp_gt@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 3), {}),
    },
    'litcmp_flipped_gt@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 2), {}),
    },
    'litcmp_ge@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 2), {}),
    },
    'litcmp_flipped_ge@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 3), {}),
    },
    'colcol_eq@4': {
        'columns_of': ('a', 'b'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (13, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')), {'__codes_of_b_in_a': '<codes of B in A>'}),
        'chosen': (),
        'in_sets': (('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')), {}),
    },
    'colcol_lt@4': {
        'columns_of': ('a', 'b'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (17, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('lt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')),
             {'__joint_rank_a_with_b': '<joint ranks of A>', '__joint_rank_b_with_a': '<joint ranks of B>'}),
        'chosen': (),
        'in_sets': (('lt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')), {}),
    },
    'colcol_ge@4': {
        'columns_of': ('a', 'b'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (16, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('ge', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')),
             {'__joint_rank_a_with_b': '<joint ranks of A>', '__joint_rank_b_with_a': '<joint ranks of B>'}),
        'chosen': (),
        'in_sets': (('ge', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')), {}),
    },
    'symlit_==@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('eq', 'a', 3), {}),
    },
    'symlit_flipped_==@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('eq', 'a', 3), {}),
    },
    'symlit_=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('eq', 'a', 3), {}),
    },
    'symlit_flipped_=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('eq', 'a', 3), {}),
    },
    'symlit_!=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ne', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('ne', 'a', 3), {}),
    },
    'symlit_flipped_!=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ne', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('ne', 'a', 3), {}),
    },
    'symlit_<>@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ne', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('ne', 'a', 3), {}),
    },
    'symlit_flipped_<>@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ne', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('ne', 'a', 3), {}),
    },
    'symlit_<@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 2), {}),
    },
    'symlit_flipped_<@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 3), {}),
    },
    'symlit_<=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 3), {}),
    },
    'symlit_flipped_<=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 2), {}),
    },
    'symlit_>@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 3), {}),
    },
    'symlit_flipped_>@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 2), {}),
    },
    'symlit_>=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ge', '__rank_a', 2), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('ge', '__rank_a', 2), {}),
    },
    'symlit_flipped_>=@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('lt', '__rank_a', 3), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_a', 3), {}),
    },
    'symnum_eq@4': {
        'columns_of': ('v',),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, 3), (13, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('=', 'v', 3), {}),
        'chosen': (),
        'in_sets': (('=', 'v', 3), {}),
    },
    'symnum_ne@4': {
        'columns_of': ('v',),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, 3), (14, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('<>', 'v', 3), {}),
        'chosen': (),
        'in_sets': (('<>', 'v', 3), {}),
    },
    'symnum_le@4': {
        'columns_of': ('w',),
        'program': ((0, 0, 0.0, 0), (1, 0, 2.5, 0), (18, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('<=', 'w', 2.5), {}),
        'chosen': (),
        'in_sets': (('<=', 'w', 2.5), {}),
    },
    'shared_eq@4': {
        'columns_of': ('s1', 's2'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (13, 0, 0.0, 0)),
        'result_type': ('raises', 'KeyError', "'s1'"),
        'lowered': (('eq', 's1', 's2'), {}),
        'chosen': (),
        'in_sets': (('eq', 's1', 's2'), {}),
    },
    'shared_lt@4': {
        'columns_of': ('s1', 's2'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (17, 0, 0.0, 0)),
        'result_type': ('raises', 'KeyError', "'s1'"),
        'lowered': (('lt', '__rank_s1', '__rank_s2'), {'__rank_s1': '<ranks of s1>', '__rank_s2': '<ranks of s2>'}),
        'chosen': (),
        'in_sets': (('lt', '__rank_s1', '__rank_s2'), {}),
    },
    'between_cols@4': {
        'columns_of': ('a', 'b', 's1'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (16, 0, 0.0, 0), (0, 0, 0.0, 0), (0, 2, 0.0, 0), (18, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': ('raises', 'KeyError', "'s1'"),
        'lowered': (('and', ('ge', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')),
              ('le', ('lookup_i32', 'a', '__joint_rank_a_with_s1'), ('lookup_i32', 's1', '__joint_rank_s1_with_a'))),
             {'__joint_rank_a_with_b': '<joint ranks of A>',
              '__joint_rank_a_with_s1': '<joint ranks of A>',
              '__joint_rank_b_with_a': '<joint ranks of B>',
              '__joint_rank_s1_with_a': '<joint ranks of S>'}),
        'chosen': (),
        'in_sets': (('and', ('ge', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')),
              ('le', ('lookup_i32', 'a', '__joint_rank_a_with_s1'), ('lookup_i32', 's1', '__joint_rank_s1_with_a'))),
             {}),
    },
    'not_between_cols@4': {
        'columns_of': ('a', 'b'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (17, 0, 0.0, 0), (0, 0, 0.0, 0), (0, 1, 0.0, 0), (15, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('or', ('lt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')),
              ('gt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a'))),
             {'__joint_rank_a_with_b': '<joint ranks of A>', '__joint_rank_b_with_a': '<joint ranks of B>'}),
        'chosen': (),
        'in_sets': (('or', ('lt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')),
              ('gt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a'))),
             {}),
    },
    'nest@4': {
        'columns_of': ('a', 'b', 'v'),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('or', ('and', ('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')), ('gt', 'v', 3)),
              ('not', ('lt', ('lookup_i32', 'b', '__joint_rank_b_with_a'), ('lookup_i32', 'a', '__joint_rank_a_with_b'))), ('eq', 'a', 3),
              ('to_int', ('ne', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')))),
             {'__codes_of_b_in_a': '<codes of B in A>', '__joint_rank_a_with_b': '<joint ranks of A>', '__joint_rank_b_with_a': '<joint ranks of B>'}),
        'chosen': (),
        'in_sets': (('or', ('and', ('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')), ('gt', 'v', 3)),
              ('not', ('lt', ('lookup_i32', 'b', '__joint_rank_b_with_a'), ('lookup_i32', 'a', '__joint_rank_a_with_b'))), ('eq', 'a', 3),
              ('to_int', ('ne', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')))),
             {}),
    },
    'litcmp_absent@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'a', -2), {}),
        'chosen': (),
        'in_sets': (('eq', 'a', -2), {}),
    },
    'litcmp_bytes@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('ne', 'a', 3), {}),
        'chosen': (),
        'in_sets': (('ne', 'a', 3), {}),
    },
    'sym_colcol_eq@4': {
        'columns_of': ('a', 'b'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (13, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')), {'__codes_of_b_in_a': '<codes of B in A>'}),
        'chosen': (),
        'in_sets': (('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a')), {}),
    },
    'sym_colcol_lt@4': {
        'columns_of': ('a', 'b'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (17, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('lt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')),
             {'__joint_rank_a_with_b': '<joint ranks of A>', '__joint_rank_b_with_a': '<joint ranks of B>'}),
        'chosen': (),
        'in_sets': (('lt', ('lookup_i32', 'a', '__joint_rank_a_with_b'), ('lookup_i32', 'b', '__joint_rank_b_with_a')), {}),
    },
    'sym_numeric@4': {
        'columns_of': ('v', 'w'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (15, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('>', 'v', 'w'), {}),
        'chosen': (),
        'in_sets': (('>', 'v', 'w'), {}),
    },
    'string_fn@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'upper'"),
        'result_type': ('raises', 'KeyError', "'upper'"),
        'lowered': (('upper', 'a'), {}),
        'chosen': (),
        'in_sets': (('upper', 'a'), {}),
    },
    'other_fn@4': {
        'columns_of': ('h', 'a', 'b'),
        'program': ('raises', 'KeyError', "'some_function'"),
        'result_type': ('raises', 'KeyError', "'some_function'"),
        'lowered': (('some_function', 'h', ('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a'))), {'__codes_of_b_in_a': '<codes of B in A>'}),
        'chosen': (),
        'in_sets': (('some_function', 'h', ('eq', 'a', ('lookup_i32', 'b', '__codes_of_b_in_a'))), {}),
    },
    'like@4': {
        'columns_of': ('a',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': (('lookup', 'a', '__like_0_a'), {'__like_0_a': "<like 'Jos%' in A>"}),
        'chosen': (),
        'in_sets': (('lookup', 'a', '__like_0_a'), {}),
    },
    'not_like@4': {
        'columns_of': ('s',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for NOT_LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for NOT_LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': (('not', ('lookup', 's', '__like_0_s')), {'__like_0_s': "<like '' in SS>"}),
        'chosen': (),
        'in_sets': (('not', ('lookup', 's', '__like_0_s')), {}),
    },
    'like_and@4': {
        'columns_of': ('s', 'v'),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': (('and', ('lookup', 's', '__like_0_s'), ('gt', 'v', 3)), {'__like_0_s': "<like 'a_c' in SS>"}),
        'chosen': (),
        'in_sets': (('and', ('lookup', 's', '__like_0_s'), ('gt', 'v', 3)), {}),
    },
    'like_not@4': {
        'columns_of': ('a',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': (('not', ('lookup', 'a', '__like_0_a')), {'__like_0_a': "<like 'ü%' in A>"}),
        'chosen': (),
        'in_sets': (('not', ('lookup', 'a', '__like_0_a')), {}),
    },
    'like_to_int@4': {
        'columns_of': ('s',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': (('to_int', ('lookup', 's', '__like_0_s')), {'__like_0_s': "<like '%b%' in SS>"}),
        'chosen': (),
        'in_sets': (('to_int', ('lookup', 's', '__like_0_s')), {}),
    },
    'like_twice@4': {
        'columns_of': ('a',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': (('or', ('lookup', 'a', '__like_0_a'), ('not', ('lookup', 'a', '__like_1_a'))),
             {'__like_0_a': "<like 'x%' in A>", '__like_1_a': "<like '%y' in A>"}),
        'chosen': (),
        'in_sets': (('or', ('lookup', 'a', '__like_0_a'), ('not', ('lookup', 'a', '__like_1_a'))), {}),
    },
    'like_one_operand@4': {
        'columns_of': ('a',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': ('raises', 'NotImplementedError', 'no GPU lowering for a LIKE node with 1 operand(s)'),
        'chosen': (),
        'in_sets': ('raises', 'NotImplementedError', 'no GPU lowering for a LIKE node with 1 operand(s)'),
    },
    'like_number_pattern@4': {
        'columns_of': ('a',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': ('raises', 'NotImplementedError', "no GPU lowering for LIKE with the pattern ('lit', 5): a string literal is required"),
        'chosen': (),
        'in_sets': ('raises', 'NotImplementedError', "no GPU lowering for LIKE with the pattern ('lit', 5): a string literal is required"),
    },
    'like_column_pattern@4': {
        'columns_of': ('a', 'b'),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': ('raises', 'NotImplementedError', "no GPU lowering for LIKE with the pattern 'b': a string literal is required"),
        'chosen': (),
        'in_sets': ('raises', 'NotImplementedError', "no GPU lowering for LIKE with the pattern 'b': a string literal is required"),
    },
    'like_numeric_column@4': {
        'columns_of': ('v',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': ('raises', 'TypeError', "LIKE needs a string column, 'v' is int64"),
        'chosen': (),
        'in_sets': ('raises', 'TypeError', "LIKE needs a string column, 'v' is int64"),
    },
    'like_unknown_column@4': {
        'columns_of': ('zz',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': ('raises', 'NotImplementedError', "no GPU lowering for LIKE over 'zz': the operand must be a column"),
        'chosen': (),
        'in_sets': ('raises', 'NotImplementedError', "no GPU lowering for LIKE over 'zz': the operand must be a column"),
    },
    'like_expression_operand@4': {
        'columns_of': ('a',),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': ('raises', 'NotImplementedError', "no GPU lowering for LIKE over ('upper', 'a'): the operand must be a column"),
        'chosen': (),
        'in_sets': ('raises', 'NotImplementedError', "no GPU lowering for LIKE over ('upper', 'a'): the operand must be a column"),
    },
    'in_3@1': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (1, 2, 3)), {}),
        'chosen': (('in', 'k', 3),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 3>'}),
    },
    'in_3@4': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (1, 2, 3)), {}),
        'chosen': (),
        'in_sets': (('in', 'k', (1, 2, 3)), {}),
    },
    'in_3@17': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (1, 2, 3)), {}),
        'chosen': (),
        'in_sets': (('in', 'k', (1, 2, 3)), {}),
    },
    'in_4@1': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 4), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (1, 2, 3, 4)), {}),
        'chosen': (('in', 'k', 4),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 4>'}),
    },
    'in_4@4': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 4), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (1, 2, 3, 4)), {}),
        'chosen': (('in', 'k', 4),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 4>'}),
    },
    'in_4@17': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 4), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (1, 2, 3, 4)), {}),
        'chosen': (),
        'in_sets': (('in', 'k', (1, 2, 3, 4)), {}),
    },
    'in_16@1': {
        'columns_of': ('k',),
        'program': ('long', 63, '430739ca705b'),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
        'chosen': (('in', 'k', 16),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 16>'}),
    },
    'in_16@4': {
        'columns_of': ('k',),
        'program': ('long', 63, '430739ca705b'),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
        'chosen': (('in', 'k', 16),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 16>'}),
    },
    'in_16@17': {
        'columns_of': ('k',),
        'program': ('long', 63, '430739ca705b'),
        'result_type': 'uint8',
        'lowered': (('in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
        'chosen': (),
        'in_sets': (('in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
    },
    'not_in_16@1': {
        'columns_of': ('k',),
        'program': ('long', 63, 'ddf9b05feac4'),
        'result_type': 'uint8',
        'lowered': (('not_in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
        'chosen': (('not_in', 'k', 16),),
        'in_sets': (('eq', '__in_0', 0), {'__in_0': '<mask of k over 16>'}),
    },
    'not_in_16@4': {
        'columns_of': ('k',),
        'program': ('long', 63, 'ddf9b05feac4'),
        'result_type': 'uint8',
        'lowered': (('not_in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
        'chosen': (('not_in', 'k', 16),),
        'in_sets': (('eq', '__in_0', 0), {'__in_0': '<mask of k over 16>'}),
    },
    'not_in_16@17': {
        'columns_of': ('k',),
        'program': ('long', 63, 'ddf9b05feac4'),
        'result_type': 'uint8',
        'lowered': (('not_in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
        'chosen': (),
        'in_sets': (('not_in', 'k', (100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115)), {}),
    },
    'in_17_and@1': {
        'columns_of': ('k',),
        'program': ('long', 71, '4f07332de81b'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'k', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), ('gt', 'k', 3)), {}),
        'chosen': (('in', 'k', 17),),
        'in_sets': (('and', ('ne', '__in_0', 0), ('gt', 'k', 3)), {'__in_0': '<mask of k over 17>'}),
    },
    'in_17_and@4': {
        'columns_of': ('k',),
        'program': ('long', 71, '4f07332de81b'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'k', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), ('gt', 'k', 3)), {}),
        'chosen': (('in', 'k', 17),),
        'in_sets': (('and', ('ne', '__in_0', 0), ('gt', 'k', 3)), {'__in_0': '<mask of k over 17>'}),
    },
    'in_17_and@17': {
        'columns_of': ('k',),
        'program': ('long', 71, '4f07332de81b'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'k', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), ('gt', 'k', 3)), {}),
        'chosen': (('in', 'k', 17),),
        'in_sets': (('and', ('ne', '__in_0', 0), ('gt', 'k', 3)), {'__in_0': '<mask of k over 17>'}),
    },
    'not_in_17@1': {
        'columns_of': ('k',),
        'program': ('long', 67, 'fab102fc6769'),
        'result_type': 'uint8',
        'lowered': (('not_in', 'k', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('not_in', 'k', 17),),
        'in_sets': (('eq', '__in_0', 0), {'__in_0': '<mask of k over 17>'}),
    },
    'not_in_17@4': {
        'columns_of': ('k',),
        'program': ('long', 67, 'fab102fc6769'),
        'result_type': 'uint8',
        'lowered': (('not_in', 'k', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('not_in', 'k', 17),),
        'in_sets': (('eq', '__in_0', 0), {'__in_0': '<mask of k over 17>'}),
    },
    'not_in_17@17': {
        'columns_of': ('k',),
        'program': ('long', 67, 'fab102fc6769'),
        'result_type': 'uint8',
        'lowered': (('not_in', 'k', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('not_in', 'k', 17),),
        'in_sets': (('eq', '__in_0', 0), {'__in_0': '<mask of k over 17>'}),
    },
    'in_two_tens@1': {
        'columns_of': ('x', 'y'),
        'program': ('long', 83, '985699b1829d'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('in', 'y', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10))), {}),
        'chosen': (('in', 'x', 10), ('in', 'y', 11)),
        'in_sets': (('and', ('ne', '__in_0', 0), ('ne', '__in_1', 0)), {'__in_0': '<mask of x over 10>', '__in_1': '<mask of y over 11>'}),
    },
    'in_two_tens@4': {
        'columns_of': ('x', 'y'),
        'program': ('long', 83, '985699b1829d'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('in', 'y', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10))), {}),
        'chosen': (('in', 'x', 10), ('in', 'y', 11)),
        'in_sets': (('and', ('ne', '__in_0', 0), ('ne', '__in_1', 0)), {'__in_0': '<mask of x over 10>', '__in_1': '<mask of y over 11>'}),
    },
    'in_two_tens@17': {
        'columns_of': ('x', 'y'),
        'program': ('long', 83, '985699b1829d'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('in', 'y', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10))), {}),
        'chosen': (('in', 'y', 11),),
        'in_sets': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('ne', '__in_0', 0)), {'__in_0': '<mask of y over 11>'}),
    },
    'in_three@1': {
        'columns_of': ('x', 'y'),
        'program': ('long', 131, '7c7b9a9860db'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('in', 'y', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)),
              ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11))),
             {}),
        'chosen': (('in', 'x', 10), ('in', 'y', 11), ('in', 'x', 12)),
        'in_sets': (('and', ('ne', '__in_0', 0), ('ne', '__in_1', 0), ('ne', '__in_2', 0)),
             {'__in_0': '<mask of x over 10>', '__in_1': '<mask of y over 11>', '__in_2': '<mask of x over 12>'}),
    },
    'in_three@4': {
        'columns_of': ('x', 'y'),
        'program': ('long', 131, '7c7b9a9860db'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('in', 'y', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)),
              ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11))),
             {}),
        'chosen': (('in', 'x', 10), ('in', 'y', 11), ('in', 'x', 12)),
        'in_sets': (('and', ('ne', '__in_0', 0), ('ne', '__in_1', 0), ('ne', '__in_2', 0)),
             {'__in_0': '<mask of x over 10>', '__in_1': '<mask of y over 11>', '__in_2': '<mask of x over 12>'}),
    },
    'in_three@17': {
        'columns_of': ('x', 'y'),
        'program': ('long', 131, '7c7b9a9860db'),
        'result_type': 'uint8',
        'lowered': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('in', 'y', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)),
              ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11))),
             {}),
        'chosen': (('in', 'x', 12), ('in', 'y', 11)),
        'in_sets': (('and', ('in', 'x', (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)), ('ne', '__in_0', 0), ('ne', '__in_1', 0)),
             {'__in_0': '<mask of y over 11>', '__in_1': '<mask of x over 12>'}),
    },
    'in_mixed@1': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (14, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 4), (14, 0, 0.0, 0), (19, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 5),
             (14, 0, 0.0, 0), (19, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 6), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('or', ('in', 'k', (1, 2)), ('not_in', 'k', (3, 4, 5)), ('in', 'k', (6,))), {}),
        'chosen': (('in', 'k', 2), ('not_in', 'k', 3), ('in', 'k', 1)),
        'in_sets': (('or', ('ne', '__in_0', 0), ('eq', '__in_1', 0), ('ne', '__in_2', 0)),
             {'__in_0': '<mask of k over 2>', '__in_1': '<mask of k over 3>', '__in_2': '<mask of k over 1>'}),
    },
    'in_mixed@4': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (14, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 4), (14, 0, 0.0, 0), (19, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 5),
             (14, 0, 0.0, 0), (19, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 6), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('or', ('in', 'k', (1, 2)), ('not_in', 'k', (3, 4, 5)), ('in', 'k', (6,))), {}),
        'chosen': (),
        'in_sets': (('or', ('in', 'k', (1, 2)), ('not_in', 'k', (3, 4, 5)), ('in', 'k', (6,))), {}),
    },
    'in_mixed@17': {
        'columns_of': ('k',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 1), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 2), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (2, 1, 0.0, 3), (14, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 4), (14, 0, 0.0, 0), (19, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 5),
             (14, 0, 0.0, 0), (19, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 1, 0.0, 6), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('or', ('in', 'k', (1, 2)), ('not_in', 'k', (3, 4, 5)), ('in', 'k', (6,))), {}),
        'chosen': (),
        'in_sets': (('or', ('in', 'k', (1, 2)), ('not_in', 'k', (3, 4, 5)), ('in', 'k', (6,))), {}),
    },
    'in_1000@1': {
        'columns_of': ('k',),
        'program': ('long', 3999, 'c22da466feb4'),
        'result_type': 'uint8',
        'lowered': (('in', 'k', ('long', 1000, 'f7903fa1ed44')), {}),
        'chosen': (('in', 'k', 1000),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 1000>'}),
    },
    'in_1000@4': {
        'columns_of': ('k',),
        'program': ('long', 3999, 'c22da466feb4'),
        'result_type': 'uint8',
        'lowered': (('in', 'k', ('long', 1000, 'f7903fa1ed44')), {}),
        'chosen': (('in', 'k', 1000),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 1000>'}),
    },
    'in_1000@17': {
        'columns_of': ('k',),
        'program': ('long', 3999, 'c22da466feb4'),
        'result_type': 'uint8',
        'lowered': (('in', 'k', ('long', 1000, 'f7903fa1ed44')), {}),
        'chosen': (('in', 'k', 1000),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 1000>'}),
    },
    'in_1000_expr@1': {
        'columns_of': ('k',),
        'program': ('long', 6000, 'ee45ea7a6ca6'),
        'result_type': 'int64',
        'lowered': (('to_int', ('not_in', ('add', 'k', 1), ('long', 1000, 'f7903fa1ed44'))), {}),
        'chosen': (('not_in', ('add', 'k', 1), 1000),),
        'in_sets': (('to_int', ('eq', '__in_0', 0)), {'__in_0': "<mask of <projected ('add', 'k', 1)> over 1000>"}),
    },
    'in_1000_expr@4': {
        'columns_of': ('k',),
        'program': ('long', 6000, 'ee45ea7a6ca6'),
        'result_type': 'int64',
        'lowered': (('to_int', ('not_in', ('add', 'k', 1), ('long', 1000, 'f7903fa1ed44'))), {}),
        'chosen': (('not_in', ('add', 'k', 1), 1000),),
        'in_sets': (('to_int', ('eq', '__in_0', 0)), {'__in_0': "<mask of <projected ('add', 'k', 1)> over 1000>"}),
    },
    'in_1000_expr@17': {
        'columns_of': ('k',),
        'program': ('long', 6000, 'ee45ea7a6ca6'),
        'result_type': 'int64',
        'lowered': (('to_int', ('not_in', ('add', 'k', 1), ('long', 1000, 'f7903fa1ed44'))), {}),
        'chosen': (('not_in', ('add', 'k', 1), 1000),),
        'in_sets': (('to_int', ('eq', '__in_0', 0)), {'__in_0': "<mask of <projected ('add', 'k', 1)> over 1000>"}),
    },
    'in_f16_operand@1': {
        'columns_of': ('h8',),
        'program': ('long', 84, 'bfc759e78d8e'),
        'result_type': ('raises', 'TypeError', 'IN over a float16 value: a set probe takes no float16 operand (cast it with to_float())'),
        'lowered': (('in', ('sqrt', 'h8'), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('in', ('sqrt', 'h8'), 17),),
        'in_sets': ('raises', 'KeyError', "'h8'"),
    },
    'in_f16_operand@4': {
        'columns_of': ('h8',),
        'program': ('long', 84, 'bfc759e78d8e'),
        'result_type': ('raises', 'TypeError', 'IN over a float16 value: a set probe takes no float16 operand (cast it with to_float())'),
        'lowered': (('in', ('sqrt', 'h8'), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('in', ('sqrt', 'h8'), 17),),
        'in_sets': ('raises', 'KeyError', "'h8'"),
    },
    'in_f16_operand@17': {
        'columns_of': ('h8',),
        'program': ('long', 84, 'bfc759e78d8e'),
        'result_type': ('raises', 'TypeError', 'IN over a float16 value: a set probe takes no float16 operand (cast it with to_float())'),
        'lowered': (('in', ('sqrt', 'h8'), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('in', ('sqrt', 'h8'), 17),),
        'in_sets': ('raises', 'KeyError', "'h8'"),
    },
    'in_predicate_operand@1': {
        'columns_of': ('k',),
        'program': ('long', 101, '6daa4f355bd9'),
        'result_type': ('raises', 'TypeError', 'IN over a predicate: the operand of a set probe must be a numeric value (cast it with to_int())'),
        'lowered': (('in', ('gt', 'k', 1), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('in', ('gt', 'k', 1), 17),),
        'in_sets': ('raises', 'TypeError', 'IN over a predicate: the operand of a set probe must be a numeric value (cast it with to_int())'),
    },
    'in_predicate_operand@4': {
        'columns_of': ('k',),
        'program': ('long', 101, '6daa4f355bd9'),
        'result_type': ('raises', 'TypeError', 'IN over a predicate: the operand of a set probe must be a numeric value (cast it with to_int())'),
        'lowered': (('in', ('gt', 'k', 1), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('in', ('gt', 'k', 1), 17),),
        'in_sets': ('raises', 'TypeError', 'IN over a predicate: the operand of a set probe must be a numeric value (cast it with to_int())'),
    },
    'in_predicate_operand@17': {
        'columns_of': ('k',),
        'program': ('long', 101, '6daa4f355bd9'),
        'result_type': ('raises', 'TypeError', 'IN over a predicate: the operand of a set probe must be a numeric value (cast it with to_int())'),
        'lowered': (('in', ('gt', 'k', 1), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)), {}),
        'chosen': (('in', ('gt', 'k', 1), 17),),
        'in_sets': ('raises', 'TypeError', 'IN over a predicate: the operand of a set probe must be a numeric value (cast it with to_int())'),
    },
    'in_floats@1': {
        'columns_of': ('w',),
        'program': ((0, 0, 0.0, 0), (1, 1, 1.0, 0), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (1, 1, 2.5, 0), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (1, 1, 3.0, 0), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'w', (1, 2.5, 3)), {}),
        'chosen': (('in', 'w', 3),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of w over 3>'}),
    },
    'in_floats@4': {
        'columns_of': ('w',),
        'program': ((0, 0, 0.0, 0), (1, 1, 1.0, 0), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (1, 1, 2.5, 0), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (1, 1, 3.0, 0), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'w', (1, 2.5, 3)), {}),
        'chosen': (),
        'in_sets': (('in', 'w', (1, 2.5, 3)), {}),
    },
    'in_floats@17': {
        'columns_of': ('w',),
        'program': ((0, 0, 0.0, 0), (1, 1, 1.0, 0), (13, 0, 0.0, 0), (0, 0, 0.0, 0), (1, 1, 2.5, 0), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 0, 0.0, 0),
             (1, 1, 3.0, 0), (13, 0, 0.0, 0), (20, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('in', 'w', (1, 2.5, 3)), {}),
        'chosen': (),
        'in_sets': (('in', 'w', (1, 2.5, 3)), {}),
    },
    'in_empty@1': {
        'columns_of': ('k',),
        'program': ('raises', 'ValueError', 'IN with an empty list'),
        'result_type': ('raises', 'ValueError', 'IN with an empty list'),
        'lowered': (('in', 'k', ()), {}),
        'chosen': (),
        'in_sets': (('in', 'k', ()), {}),
    },
    'in_empty@4': {
        'columns_of': ('k',),
        'program': ('raises', 'ValueError', 'IN with an empty list'),
        'result_type': ('raises', 'ValueError', 'IN with an empty list'),
        'lowered': (('in', 'k', ()), {}),
        'chosen': (),
        'in_sets': (('in', 'k', ()), {}),
    },
    'in_empty@17': {
        'columns_of': ('k',),
        'program': ('raises', 'ValueError', 'IN with an empty list'),
        'result_type': ('raises', 'ValueError', 'IN with an empty list'),
        'lowered': (('in', 'k', ()), {}),
        'chosen': (),
        'in_sets': (('in', 'k', ()), {}),
    },
    'in_dict_strs@1': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'result_type': 'uint8',
        'lowered': (('in', 'a', (3, 5)), {}),
        'chosen': (('in', 'a', 3),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of a over 2>'}),
    },
    'in_dict_strs@4': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'result_type': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'lowered': (('in', 'a', (3, 5)), {}),
        'chosen': (),
        'in_sets': (('in', 'a', (3, 5)), {}),
    },
    'in_dict_strs@17': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'result_type': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'lowered': (('in', 'a', (3, 5)), {}),
        'chosen': (),
        'in_sets': (('in', 'a', (3, 5)), {}),
    },
    'in_dict_lits@1': {
        'columns_of': ('a',),
        'program': ('raises', 'TypeError', "int() argument must be a string, a bytes-like object or a real number, not 'tuple'"),
        'result_type': 'uint8',
        'lowered': (('not_in', 'a', (3,)), {}),
        'chosen': (('not_in', 'a', 2),),
        'in_sets': (('eq', '__in_0', 0), {'__in_0': '<mask of a over 1>'}),
    },
    'in_dict_lits@4': {
        'columns_of': ('a',),
        'program': ('raises', 'TypeError', "int() argument must be a string, a bytes-like object or a real number, not 'tuple'"),
        'result_type': ('raises', 'TypeError', "int() argument must be a string, a bytes-like object or a real number, not 'tuple'"),
        'lowered': (('not_in', 'a', (3,)), {}),
        'chosen': (),
        'in_sets': (('not_in', 'a', (3,)), {}),
    },
    'in_dict_lits@17': {
        'columns_of': ('a',),
        'program': ('raises', 'TypeError', "int() argument must be a string, a bytes-like object or a real number, not 'tuple'"),
        'result_type': ('raises', 'TypeError', "int() argument must be a string, a bytes-like object or a real number, not 'tuple'"),
        'lowered': (('not_in', 'a', (3,)), {}),
        'chosen': (),
        'in_sets': (('not_in', 'a', (3,)), {}),
    },
    'in_dict_none_held@1': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Oslo'"),
        'result_type': 'uint8',
        'lowered': (('in', 'a', (-2,)), {}),
        'chosen': (('in', 'a', 1),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of a over 1>'}),
    },
    'in_dict_none_held@4': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Oslo'"),
        'result_type': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Oslo'"),
        'lowered': (('in', 'a', (-2,)), {}),
        'chosen': (),
        'in_sets': (('in', 'a', (-2,)), {}),
    },
    'in_dict_none_held@17': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Oslo'"),
        'result_type': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Oslo'"),
        'lowered': (('in', 'a', (-2,)), {}),
        'chosen': (),
        'in_sets': (('in', 'a', (-2,)), {}),
    },
    'in_dict_long@1': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'result_type': 'uint8',
        'lowered': (('in', 'a', (3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5)), {}),
        'chosen': (('in', 'a', 20),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of a over 20>'}),
    },
    'in_dict_long@4': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'result_type': 'uint8',
        'lowered': (('in', 'a', (3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5)), {}),
        'chosen': (('in', 'a', 20),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of a over 20>'}),
    },
    'in_dict_long@17': {
        'columns_of': ('a',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'Berlin'"),
        'result_type': 'uint8',
        'lowered': (('in', 'a', (3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5)), {}),
        'chosen': (('in', 'a', 20),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of a over 20>'}),
    },
    'scalar_sqrt@4': {
        'columns_of': ('total',),
        'program': ((0, 0, 0.0, 0), (26, 0, 0.0, 0)),
        'result_type': 'double',
        'lowered': (('sqrt', 'total'), {}),
        'chosen': (),
        'in_sets': (('sqrt', 'total'), {}),
    },
    'scalar_to_int@4': {
        'columns_of': ('lat',),
        'program': ((0, 0, 0.0, 0), (27, 0, 0.0, 0), (2, 0, 0.0, 100000), (5, 0, 0.0, 0), (35, 0, 0.0, 0)),
        'result_type': 'int64',
        'lowered': (('to_int', ('mul', ('sin', 'lat'), 100000)), {}),
        'chosen': (),
        'in_sets': (('to_int', ('mul', ('sin', 'lat'), 100000)), {}),
    },
    'scalar_pi@4': {
        'columns_of': ('fare',),
        'program': ((0, 0, 0.0, 0), (1, 0, 3.141592653589793, 0), (3, 0, 0.0, 0)),
        'result_type': 'float',
        'lowered': (('add', 'fare', ('pi',)), {}),
        'chosen': (),
        'in_sets': (('add', 'fare', ('pi',)), {}),
    },
    'scalar_abs@4': {
        'columns_of': ('total', 'tip'),
        'program': ((0, 0, 0.0, 0), (0, 1, 0.0, 0), (4, 0, 0.0, 0), (25, 0, 0.0, 0)),
        'result_type': 'double',
        'lowered': (('abs', ('sub', 'total', 'tip')), {}),
        'chosen': (),
        'in_sets': (('abs', ('sub', 'total', 'tip')), {}),
    },
    'scalar_power@4': {
        'columns_of': ('fare',),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, 2), (33, 0, 0.0, 0)),
        'result_type': 'float',
        'lowered': (('power', 'fare', 2), {}),
        'chosen': (),
        'in_sets': (('power', 'fare', 2), {}),
    },
    'scalar_to_float@4': {
        'columns_of': ('n',),
        'program': ((0, 0, 0.0, 0), (34, 0, 0.0, 0)),
        'result_type': 'double',
        'lowered': (('to_float', 'n'), {}),
        'chosen': (),
        'in_sets': (('to_float', 'n'), {}),
    },
    'scalar_to_bool@4': {
        'columns_of': ('n',),
        'program': ((0, 0, 0.0, 0), (36, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('to_bool', 'n'), {}),
        'chosen': (),
        'in_sets': (('to_bool', 'n'), {}),
    },
    'scalar_e@4': {
        'columns_of': ('lat',),
        'program': ((1, 0, 2.718281828459045, 0), (0, 0, 0.0, 0), (28, 0, 0.0, 0), (5, 0, 0.0, 0)),
        'result_type': 'double',
        'lowered': (('mul', ('e',), ('cos', 'lat')), {}),
        'chosen': (),
        'in_sets': (('mul', ('e',), ('cos', 'lat')), {}),
    },
    'fold_sqrt@4': {
        'columns_of': ('v',),
        'program': ((1, 1, 2.0, 0), (0, 0, 0.0, 0), (5, 0, 0.0, 0)),
        'result_type': 'double',
        'lowered': (('mul', ('sqrt', 4), 'v'), {}),
        'chosen': (),
        'in_sets': (('mul', ('sqrt', 4), 'v'), {}),
    },
    'fold_nested@4': {
        'columns_of': ('v',),
        'program': ((0, 0, 0.0, 0), (2, 1, 0.0, 3), (3, 0, 0.0, 0)),
        'result_type': 'int64',
        'lowered': (('add', 'v', ('to_int', ('log10', 1000.0))), {}),
        'chosen': (),
        'in_sets': (('add', 'v', ('to_int', ('log10', 1000.0))), {}),
    },
    'fold_negative_power@4': {
        'columns_of': (),
        'program': ('raises', 'ValueError', 'Integers to negative integer powers are not allowed.'),
        'result_type': ('raises', 'ValueError', 'Integers to negative integer powers are not allowed.'),
        'lowered': (('power', 2, -1), {}),
        'chosen': (),
        'in_sets': (('power', 2, -1), {}),
    },
    'power_negative_literal@4': {
        'columns_of': ('i',),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, -2), (33, 0, 0.0, 0)),
        'result_type': ('raises', 'ValueError', 'Integers to negative integer powers are not allowed.'),
        'lowered': (('power', 'i', -2), {}),
        'chosen': (),
        'in_sets': (('power', 'i', -2), {}),
    },
    'power_folded_exponent@4': {
        'columns_of': ('i',),
        'program': ((2, 0, 0.0, 1), (0, 0, 0.0, 0), (25, 0, 0.0, 0), (2, 1, 0.0, -3), (33, 0, 0.0, 0), (3, 0, 0.0, 0)),
        'result_type': ('raises', 'ValueError', 'Integers to negative integer powers are not allowed.'),
        'lowered': (('add', 1, ('power', ('abs', 'i'), ('to_int', -3.5))), {}),
        'chosen': (),
        'in_sets': (('add', 1, ('power', ('abs', 'i'), ('to_int', -3.5))), {}),
    },
    'power_neg@4': {
        'columns_of': ('i',),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, 2), (8, 0, 0.0, 0), (33, 0, 0.0, 0)),
        'result_type': ('raises', 'ValueError', 'Integers to negative integer powers are not allowed.'),
        'lowered': (('power', 'i', ('neg', 2)), {}),
        'chosen': (),
        'in_sets': (('power', 'i', ('neg', 2)), {}),
    },
    'power_arity@4': {
        'columns_of': ('i',),
        'program': ('raises', 'TypeError', 'power() takes 2 argument(s), 1 given'),
        'result_type': ('raises', 'TypeError', 'power() takes 2 argument(s), 1 given'),
        'lowered': (('power', 'i'), {}),
        'chosen': (),
        'in_sets': (('power', 'i'), {}),
    },
    'bool_literal@4': {
        'columns_of': ('v',),
        'program': ('raises', 'TypeError', 'boolean literals are not arithmetic operands'),
        'result_type': ('raises', 'TypeError', 'boolean literals are not arithmetic operands'),
        'lowered': (('add', 'v', True), {}),
        'chosen': (),
        'in_sets': (('add', 'v', True), {}),
    },
    'planner_between_in@1': {
        'columns_of': ('v', 'k'),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, 10), (16, 0, 0.0, 0), (0, 0, 0.0, 0), (1, 0, 50.5, 0), (18, 0, 0.0, 0), (19, 0, 0.0, 0), (0, 1, 0.0, 0),
             (2, 1, 0.0, 4), (13, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 11), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 18),
             (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 410), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('and', ('between', 'v', 10, 50.5), ('in', 'k', (4, 11, 18, 410))), {}),
        'chosen': (('in', 'k', 4),),
        'in_sets': (('and', ('between', 'v', 10, 50.5), ('ne', '__in_0', 0)), {'__in_0': '<mask of k over 4>'}),
    },
    'planner_between_in@4': {
        'columns_of': ('v', 'k'),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, 10), (16, 0, 0.0, 0), (0, 0, 0.0, 0), (1, 0, 50.5, 0), (18, 0, 0.0, 0), (19, 0, 0.0, 0), (0, 1, 0.0, 0),
             (2, 1, 0.0, 4), (13, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 11), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 18),
             (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 410), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('and', ('between', 'v', 10, 50.5), ('in', 'k', (4, 11, 18, 410))), {}),
        'chosen': (('in', 'k', 4),),
        'in_sets': (('and', ('between', 'v', 10, 50.5), ('ne', '__in_0', 0)), {'__in_0': '<mask of k over 4>'}),
    },
    'planner_between_in@17': {
        'columns_of': ('v', 'k'),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, 10), (16, 0, 0.0, 0), (0, 0, 0.0, 0), (1, 0, 50.5, 0), (18, 0, 0.0, 0), (19, 0, 0.0, 0), (0, 1, 0.0, 0),
             (2, 1, 0.0, 4), (13, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 11), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 18),
             (13, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 410), (13, 0, 0.0, 0), (20, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('and', ('between', 'v', 10, 50.5), ('in', 'k', (4, 11, 18, 410))), {}),
        'chosen': (),
        'in_sets': (('and', ('between', 'v', 10, 50.5), ('in', 'k', (4, 11, 18, 410))), {}),
    },
    'planner_not_between_not_in@1': {
        'columns_of': ('i', 'g'),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, -900), (17, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 0, 0.0, 900), (15, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0),
             (2, 1, 0.0, 0), (14, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 6), (14, 0, 0.0, 0), (19, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('and', ('not_between', 'i', -900, 900), ('not_in', 'g', (0, 6))), {}),
        'chosen': (('not_in', 'g', 2),),
        'in_sets': (('and', ('not_between', 'i', -900, 900), ('eq', '__in_0', 0)), {'__in_0': '<mask of g over 2>'}),
    },
    'planner_not_between_not_in@4': {
        'columns_of': ('i', 'g'),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, -900), (17, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 0, 0.0, 900), (15, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0),
             (2, 1, 0.0, 0), (14, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 6), (14, 0, 0.0, 0), (19, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('and', ('not_between', 'i', -900, 900), ('not_in', 'g', (0, 6))), {}),
        'chosen': (),
        'in_sets': (('and', ('not_between', 'i', -900, 900), ('not_in', 'g', (0, 6))), {}),
    },
    'planner_not_between_not_in@17': {
        'columns_of': ('i', 'g'),
        'program': ((0, 0, 0.0, 0), (2, 0, 0.0, -900), (17, 0, 0.0, 0), (0, 0, 0.0, 0), (2, 0, 0.0, 900), (15, 0, 0.0, 0), (20, 0, 0.0, 0), (0, 1, 0.0, 0),
             (2, 1, 0.0, 0), (14, 0, 0.0, 0), (0, 1, 0.0, 0), (2, 1, 0.0, 6), (14, 0, 0.0, 0), (19, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('and', ('not_between', 'i', -900, 900), ('not_in', 'g', (0, 6))), {}),
        'chosen': (),
        'in_sets': (('and', ('not_between', 'i', -900, 900), ('not_in', 'g', (0, 6))), {}),
    },
    'planner_is_null@4': {
        'columns_of': ('y',),
        'program': ((22, 0, 0.0, 0),),
        'result_type': 'uint8',
        'lowered': (('is_null', 'y'), {}),
        'chosen': (),
        'in_sets': (('is_null', 'y'), {}),
    },
    'planner_is_not_null@4': {
        'columns_of': ('tip',),
        'program': ((23, 0, 0.0, 0), (0, 0, 0.0, 0), (1, 0, 0.5, 0), (15, 0, 0.0, 0), (19, 0, 0.0, 0)),
        'result_type': 'uint8',
        'lowered': (('and', ('is_not_null', 'tip'), ('gt', 'tip', 0.5)), {}),
        'chosen': (),
        'in_sets': (('and', ('is_not_null', 'tip'), ('gt', 'tip', 0.5)), {}),
    },
    'planner_arith@4': {
        'columns_of': ('total', 'tip'),
        'program': ((2, 0, 0.0, 1), (0, 0, 0.0, 0), (4, 0, 0.0, 0), (2, 0, 0.0, 2), (0, 1, 0.0, 0), (3, 0, 0.0, 0), (5, 0, 0.0, 0)),
        'result_type': 'double',
        'lowered': (('mul', ('sub', 1, 'total'), ('add', 2, 'tip')), {}),
        'chosen': (),
        'in_sets': (('mul', ('sub', 1, 'total'), ('add', 2, 'tip')), {}),
    },
    'column@4': {
        'columns_of': ('v',),
        'program': ((0, 0, 0.0, 0),),
        'result_type': 'int64',
        'lowered': ('v', {}),
        'chosen': (),
        'in_sets': ('v', {}),
    },
    'number@4': {
        'columns_of': (),
        'program': ((2, 0, 0.0, 7),),
        'result_type': 'int64',
        'lowered': (7, {}),
        'chosen': (),
        'in_sets': (7, {}),
    },
    'strong@4': {
        'columns_of': ('v',),
        'program': ((0, 0, 0.0, 0), (1, 1, 2.5, 0), (3, 0, 0.0, 0)),
        'result_type': 'double',
        'lowered': (('add', 'v', ('strong', 2.5)), {}),
        'chosen': (),
        'in_sets': (('add', 'v', ('strong', 2.5)), {}),
    },
    'lookup@4': {
        'columns_of': ('s', '__t'),
        'program': ((37, 0, 0.0, 1), (21, 0, 0.0, 0)),
        'result_type': ('raises', 'KeyError', "'__t'"),
        'lowered': (('not', ('lookup', 's', '__t')), {}),
        'chosen': (),
        'in_sets': (('not', ('lookup', 's', '__t')), {}),
    },
    'lookup_i32@4': {
        'columns_of': ('a', 'b', '__t'),
        'program': ((0, 0, 0.0, 0), (38, 1, 0.0, 2), (13, 0, 0.0, 0)),
        'result_type': ('raises', 'KeyError', "'__t'"),
        'lowered': ('raises', 'TypeError',
             "cannot compare the string column 'a' with ('lookup_i32', 'b', '__t'): only a string / binary literal or another such column"),
        'chosen': (),
        'in_sets': ('raises', 'TypeError',
             "cannot compare the string column 'a' with ('lookup_i32', 'b', '__t'): only a string / binary literal or another such column"),
    },
    'unknown_operator@4': {
        'columns_of': ('v',),
        'program': ('raises', 'KeyError', "'frobnicate'"),
        'result_type': ('raises', 'KeyError', "'frobnicate'"),
        'lowered': (('frobnicate', 'v'), {}),
        'chosen': (),
        'in_sets': (('frobnicate', 'v'), {}),
    },
    'lit_alone@4': {
        'columns_of': ('v',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 'v', ('lit', 'x')), {}),
        'chosen': (),
        'in_sets': (('eq', 'v', ('lit', 'x')), {}),
    },
    'trap_value_list_names_columns@1': {
        'columns_of': ('k',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'a'"),
        'result_type': 'uint8',
        'lowered': (('in', 'k', ('a', 'b')), {}),
        'chosen': (('in', 'k', 2),),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': '<mask of k over 2>'}),
    },
    'trap_value_list_names_columns@4': {
        'columns_of': ('k',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'a'"),
        'result_type': ('raises', 'ValueError', "invalid literal for int() with base 10: 'a'"),
        'lowered': (('in', 'k', ('a', 'b')), {}),
        'chosen': (),
        'in_sets': (('in', 'k', ('a', 'b')), {}),
    },
    'trap_value_list_names_columns@17': {
        'columns_of': ('k',),
        'program': ('raises', 'ValueError', "invalid literal for int() with base 10: 'a'"),
        'result_type': ('raises', 'ValueError', "invalid literal for int() with base 10: 'a'"),
        'lowered': (('in', 'k', ('a', 'b')), {}),
        'chosen': (),
        'in_sets': (('in', 'k', ('a', 'b')), {}),
    },
    'trap_literal_names_a_column@4': {
        'columns_of': ('s',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('eq', 's', -2), {}),
        'chosen': (),
        'in_sets': (('eq', 's', -2), {}),
    },
    'trap_strong_beside_like@4': {
        'columns_of': ('a', 'v'),
        'program': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'result_type': ('raises', 'NotImplementedError',
             'no GPU lowering for LIKE outside a FilterOperator / ProjectOperator / AggregateOperator (they turn it into a dictionary lookup)'),
        'lowered': (('and', ('lookup', 'a', '__like_0_a'), ('gt', 'v', ('strong', 3))), {'__like_0_a': "<like 'x%' in A>"}),
        'chosen': (),
        'in_sets': (('and', ('lookup', 'a', '__like_0_a'), ('gt', 'v', ('strong', 3))), {}),
    },
    'trap_between_dictionary_literals@4': {
        'columns_of': ('a',),
        'program': ('raises', 'KeyError', "'lit'"),
        'result_type': ('raises', 'KeyError', "'lit'"),
        'lowered': (('and', ('ge', '__rank_a', 2), ('lt', '__rank_a', 3)), {'__rank_a': '<ranks of a>'}),
        'chosen': (),
        'in_sets': (('and', ('ge', '__rank_a', 2), ('lt', '__rank_a', 3)), {}),
    },
    'trap_nested_in@1': {
        'columns_of': ('k',),
        'program': ('long', 45, '0e7ba9df73fa'),
        'result_type': 'uint8',
        'lowered': (('in', ('to_int', ('in', 'k', (1, 2, 3, 4, 5))), (0, 1)), {}),
        'chosen': (('in', ('to_int', ('in', 'k', (1, 2, 3, 4, 5))), 2), ('in', 'k', 5)),
        'in_sets': (('ne', '__in_0', 0), {'__in_0': "<mask of <projected ('to_int', ('in', 'k', (1, 2, 3, 4, 5)))> over 2>"}),
    },
    'trap_nested_in@4': {
        'columns_of': ('k',),
        'program': ('long', 45, '0e7ba9df73fa'),
        'result_type': 'uint8',
        'lowered': (('in', ('to_int', ('in', 'k', (1, 2, 3, 4, 5))), (0, 1)), {}),
        'chosen': (('in', 'k', 5),),
        'in_sets': (('in', ('to_int', ('ne', '__in_0', 0)), (0, 1)), {'__in_0': '<mask of k over 5>'}),
    },
    'trap_nested_in@17': {
        'columns_of': ('k',),
        'program': ('long', 45, '0e7ba9df73fa'),
        'result_type': 'uint8',
        'lowered': (('in', ('to_int', ('in', 'k', (1, 2, 3, 4, 5))), (0, 1)), {}),
        'chosen': (),
        'in_sets': (('in', ('to_int', ('in', 'k', (1, 2, 3, 4, 5))), (0, 1)), {}),
    },
    'trap_fn@4': {
        'columns_of': ('x',),
        'program': ('raises', 'KeyError', "'fn'"),
        'result_type': ('raises', 'KeyError', "'fn'"),
        'lowered': (('fn', 'sum', ('add', 'x', 1)), {}),
        'chosen': (),
        'in_sets': (('fn', 'sum', ('add', 'x', 1)), {}),
    },
}
