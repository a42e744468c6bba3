#!/usr/bin/env python3
"""Fixtures for date() / datetime() / from_timestamp() from the reference's OWN planner + executor (build container only; ORDER BY
and the aggregates need the reference operators build() compiles).

Reuses gen_golden_planner.py's stubs and run() with gen_golden_like.py's to_ast (string literals) and has_agg, as
gen_golden_to_str.py does.  Outputs (data only): datetime_in_main.arrow (tests/golden/datetime_cases.datetime_main_table()),
datetime_<case>.arrow = the reference's result of each case of datetime_cases.CASES it can run, datetime_cases.json with the shape
of every result -- or, for a case the reference raises on here, the error.

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_datetime.py
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
from tests.golden import datetime_cases as C  # noqa: E402
import vinum  # noqa: E402


_to_ast = K.G.to_ast


def to_ast(e, alias=None):
    """["fn", name, x...] with a datetime built-in's name is the reference's FUNCTION expression of that name (parser.py builds it so)"""
    if isinstance(e, list) and e and e[0] == "fn" and e[1] in ("date", "datetime", "from_timestamp"):
        return K.Expression(K.SQLExpression.FUNCTION, tuple(to_ast(a) for a in e[2:]), function_name=e[1], alias=alias)
    return _to_ast(e, alias)


K.G.to_ast = to_ast


def main():
    warnings.simplefilter("ignore")
    vinum.set_batch_size(300)
    tables = {name: make() for name, make in C.TABLES.items()}
    K.write("datetime_in_main.arrow", tables["main"])
    meta = {"cases": {}, "raised": {}, "pyarrow": pa.__version__,
            "generator": "tests/golden/gen_golden_datetime.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in C.CASES:
        try:
            out = K.G.run(case, tables[case["table"]])
        except Exception as e:   # noqa: BLE001  (whatever the reference raises is the record)
            meta["raised"][case["name"]] = re.sub(r"_\d{3,}", "_<id>", f"{type(e).__name__}: {(str(e).splitlines() or [''])[0][:160]}")
            print(f"{case['name']:34s} RAISED {meta['raised'][case['name']]}")
            continue
        K.write(f"datetime_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:34s} {out.num_rows:6d} rows  {out.schema.names}  {[str(t) for t in out.schema.types]}")
    with open(os.path.join(HERE, "datetime_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
