#!/usr/bin/env python3
"""Fixtures for LIKE / NOT LIKE from the reference's OWN planner + executor (build container only).

Reuses gen_golden_planner.py's stubs and run(); to_ast learns the LIKE / NOT LIKE nodes and string literals, and has_agg asks
is_aggregate_func (as gen_golden_scalar_fn.py does) so to_int(...) is no aggregate.

Outputs (data only): like_in_ref.arrow (the reference's own test table, vinum/tests/conftest.py create_test_data),
like_in_main.arrow (tests/golden/like_cases.like_main_table()), like_<case>.arrow = the reference's result of each case.

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_like.py
"""
import json
import os
import sys
import warnings

import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import gen_golden_planner as G  # noqa: E402  (sets up the reference import path and stubs)
from tests.golden import like_cases as C  # noqa: E402
import vinum  # noqa: E402
from vinum.core.functions import is_aggregate_func  # noqa: E402
from vinum.parser.query import Expression, Literal, SQLExpression  # noqa: E402
from vinum.tests.conftest import create_test_data  # noqa: E402

_plain_to_ast = G.to_ast


def to_ast(e, alias=None):
    if isinstance(e, list) and e and e[0] == "lit":
        return Literal(e[1], alias)
    if isinstance(e, list) and e and e[0] in ("like", "not_like"):
        op = SQLExpression.LIKE if e[0] == "like" else SQLExpression.NOT_LIKE
        return Expression(op, (to_ast(e[1]), to_ast(e[2])), alias=alias)
    return _plain_to_ast(e, alias)


def has_agg(e):
    return isinstance(e, list) and ((e[0] == "fn" and bool(is_aggregate_func(e[1]))) or any(has_agg(a) for a in e[1:]))


G.to_ast = to_ast
G.has_agg = has_agg


def write(name, table):
    with pa.OSFile(os.path.join(HERE, name), "wb") as f:
        with pa.ipc.new_file(f, table.schema) as w:
            w.write_table(table.combine_chunks())


def main():
    warnings.simplefilter("ignore")
    vinum.set_batch_size(1000)
    tables = {"ref": create_test_data()[2]._arrow_table.get_table(), "main": C.like_main_table()}
    write("like_in_ref.arrow", tables["ref"])
    write("like_in_main.arrow", tables["main"])
    meta = {"cases": {}, "pyarrow": pa.__version__,
            "generator": "tests/golden/gen_golden_like.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in C.CASES:
        out = G.run(case, tables[case["table"]])
        write(f"like_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:20s} {out.num_rows:6d} rows  {out.schema.names}")
    with open(os.path.join(HERE, "like_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
