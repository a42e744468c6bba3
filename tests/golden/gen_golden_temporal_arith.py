#!/usr/bin/env python3
"""Fixtures for temporal arithmetic, timedelta(), is_busday() and now() from the reference's OWN planner + executor (build container
only; ORDER BY and the aggregates need the reference operators build() compiles).

Reuses gen_golden_planner.py's stubs and run() with gen_golden_like.py's to_ast (string literals) and has_agg, as
gen_golden_datetime.py does.  Outputs (data only): temporal_arith_in_main.arrow
(tests/golden/temporal_arith_cases.temporal_arith_main_table()), temporal_arith_<case>.arrow = the reference's result of each case
of temporal_arith_cases.CASES it can run, temporal_arith_cases.json with the shape of every result -- or, for a case the reference
raises on here, the error.  At least two thirds of the cases must be comparable: the script fails otherwise.

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_temporal_arith.py
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
from tests.golden import temporal_arith_cases as C  # noqa: E402
import vinum  # noqa: E402

_to_ast = K.G.to_ast
_FUNCTIONS = ("date", "datetime", "from_timestamp", "timedelta", "is_busday", "now")


def to_ast(e, alias=None):
    """["fn", name, x...] with a datetime built-in's name is the reference's FUNCTION expression of that name (parser.py builds it
    so); a list of date strings -- is_busday's holidays -- and an IN list are ONE Literal holding a Python list"""
    if isinstance(e, list) and e and e[0] == "fn" and e[1] in _FUNCTIONS:
        args = [K.Literal(list(a)) if isinstance(a, list) and a and a[0] not in ("lit", "fn") and all(isinstance(x, str) for x in a) and e[1] == "is_busday"
                and i == 2 else to_ast(a) for i, a in enumerate(e[2:])]
        return K.Expression(K.SQLExpression.FUNCTION, tuple(args), function_name=e[1], alias=alias)
    return _to_ast(e, alias)


K.G.to_ast = to_ast


def main():
    warnings.simplefilter("ignore")
    vinum.set_batch_size(300)
    tables = {name: make() for name, make in C.TABLES.items()}
    K.write("temporal_arith_in_main.arrow", tables["main"])
    meta = {"cases": {}, "raised": {}, "pyarrow": pa.__version__,
            "generator": "tests/golden/gen_golden_temporal_arith.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in C.CASES:
        try:
            out = K.G.run(case, tables[case["table"]])
        except Exception as e:   # noqa: BLE001  (whatever the reference raises is the record)
            meta["raised"][case["name"]] = re.sub(r"_\d{3,}", "_<id>", f"{type(e).__name__}: {(str(e).splitlines() or [''])[0][:160]}")
            print(f"{case['name']:40s} RAISED {meta['raised'][case['name']]}")
            continue
        K.write(f"temporal_arith_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:40s} {out.num_rows:6d} rows  {out.schema.names}  {[str(t) for t in out.schema.types]}")
    with open(os.path.join(HERE, "temporal_arith_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)
    assert 3 * len(meta["cases"]) >= 2 * len(C.CASES), f"only {len(meta['cases'])} of {len(C.CASES)} cases are comparable"


if __name__ == "__main__":
    main()
