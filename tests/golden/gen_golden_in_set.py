#!/usr/bin/env python3
"""Fixtures for IN / NOT IN with long lists from the reference's OWN planner + executor (build container only).

Reuses gen_golden_planner.py's stubs, to_ast (an IN list is ONE Literal holding the Python list, parser.py:151-160) and run();
has_agg asks is_aggregate_func (as gen_golden_like.py does) so to_int(...) is no aggregate.

Outputs (data only): in_set_in.arrow (tests/golden/in_set_cases.in_set_table()), in_set_<case>.arrow = the reference's result of
each case, in_set_cases.json = their shapes.

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_in_set.py
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
from tests.golden import in_set_cases as C  # noqa: E402
import vinum  # noqa: E402
from vinum.core.functions import is_aggregate_func  # noqa: E402


def has_agg(e):
    return isinstance(e, list) and ((e[0] == "fn" and bool(is_aggregate_func(e[1]))) or any(has_agg(a) for a in e[1:]))


G.has_agg = has_agg


def write(name, table):
    with pa.OSFile(os.path.join(HERE, name), "wb") as f:
        with pa.ipc.new_file(f, table.schema) as w:
            w.write_table(table.combine_chunks())


def main():
    warnings.simplefilter("ignore")
    vinum.set_batch_size(150)       # several batches per query
    table = C.in_set_table()
    write("in_set_in.arrow", table)
    meta = {"cases": {}, "pyarrow": pa.__version__,
            "generator": "tests/golden/gen_golden_in_set.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in C.CASES:
        out = G.run(case, table)
        write(f"in_set_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:20s} {out.num_rows:6d} rows  {out.schema.names}")
    with open(os.path.join(HERE, "in_set_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
