#!/usr/bin/env python3
"""Fixtures for upper() / lower() from the reference's OWN planner + executor (build container only; ORDER BY needs the reference
operators build() compiles).

Reuses gen_golden_planner.py's stubs and run() with gen_golden_like.py's to_ast (string literals) and has_agg (to_int is no
aggregate).  Outputs (data only): strcase_in_main.arrow (tests/golden/strcase_cases.strcase_main_table()), strcase_<case>.arrow =
the reference's result of each case, strcase_cases.json.

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_strcase.py
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

from tests.golden import gen_golden_like as K  # noqa: E402  (installs its to_ast / has_agg into gen_golden_planner)
from tests.golden import strcase_cases as C  # noqa: E402
import vinum  # noqa: E402


def main():
    warnings.simplefilter("ignore")
    vinum.set_batch_size(400)
    table = C.strcase_main_table()
    K.write("strcase_in_main.arrow", table)
    meta = {"cases": {}, "pyarrow": pa.__version__,
            "generator": "tests/golden/gen_golden_strcase.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in C.CASES:
        out = K.G.run(case, table)
        K.write(f"strcase_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:20s} {out.num_rows:6d} rows  {out.schema.names}  {[str(t) for t in out.schema.types]}")
    with open(os.path.join(HERE, "strcase_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
