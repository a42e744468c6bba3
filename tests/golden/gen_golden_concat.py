#!/usr/bin/env python3
"""Fixtures for concat() from the reference's OWN planner + executor (build container only; ORDER BY and DISTINCT need the
reference operators build() compiles).

Reuses gen_golden_planner.py's stubs and run() with gen_golden_like.py's to_ast (string literals) and has_agg.  Outputs (data
only): concat_in_main.arrow (tests/golden/concat_cases.concat_main_table()), concat_<case>.arrow = the reference's result of each
case of concat_cases.CASES, concat_cases.json.  With --probe the RESTATED cases are tried too and the error the reference raises
on each is printed (nothing is written for them).

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_concat.py [--probe]
"""
import json
import os
import re
import sys
import warnings

import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import gen_golden_like as K  # noqa: E402  (installs its to_ast / has_agg into gen_golden_planner)
from tests.golden import concat_cases as C  # noqa: E402
import vinum  # noqa: E402


_to_ast = K.G.to_ast


def to_ast(e, alias=None):
    """the operator node ["concat", x, ...] is the reference's FUNCTION expression of that name (parser.py builds it for concat(...))"""
    if isinstance(e, list) and e and e[0] == "concat":
        return K.Expression(K.SQLExpression.FUNCTION, tuple(to_ast(a) for a in e[1:]), function_name="concat", alias=alias)
    if isinstance(e, list) and e and e[0] == "fn":
        return K.Expression(K.SQLExpression.FUNCTION, tuple(to_ast(a) for a in e[2:]), function_name=e[1], alias=alias)
    return _to_ast(e, alias)


K.G.to_ast = to_ast


def main():
    warnings.simplefilter("ignore")
    vinum.set_batch_size(400)
    table = C.concat_main_table()
    K.write("concat_in_main.arrow", table)
    meta = {"cases": {}, "restated": {}, "pyarrow": pa.__version__,
            "generator": "tests/golden/gen_golden_concat.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in C.CASES:
        out = K.G.run(case, table)
        K.write(f"concat_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:24s} {out.num_rows:6d} rows  {out.schema.names}  {[str(t) for t in out.schema.types]}")
    for case in C.RESTATED:
        try:
            K.G.run(case, table)
            meta["restated"][case["name"]] = "the reference ran it"
        except Exception as e:   # noqa: BLE001  (whatever the reference raises is the record)
            meta["restated"][case["name"]] = re.sub(r"concat_\d+", "concat_<id>", f"{type(e).__name__}: {(str(e).splitlines() or [''])[0][:160]}")
        if "--probe" in sys.argv:
            print(f"{case['name']:24s} {meta['restated'][case['name']]}")
    with open(os.path.join(HERE, "concat_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
