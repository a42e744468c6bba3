#!/usr/bin/env python3
"""Fixtures for comparisons of two string columns from the reference's OWN planner + executor (build container only).

Reuses gen_golden_planner.py's stubs and run(); has_agg asks is_aggregate_func (as gen_golden_like.py does) so to_int(...) is no
aggregate.  A case the reference raises on is reported and dropped: strcmp_cases.json lists what was written.

Outputs (data only): strcmp_in_main.arrow (tests/golden/strcmp_cases.strcmp_table()), strcmp_<case>.arrow = the reference's result
of each case, strcmp_cases.json.

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_strcmp.py
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
from tests.golden import strcmp_cases as C  # noqa: E402
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
    vinum.set_batch_size(16)          # three batches over the 40 rows
    table = C.strcmp_table()
    write("strcmp_in_main.arrow", table)
    meta = {"cases": {}, "dropped": {}, "pyarrow": pa.__version__,
            "generator": "tests/golden/gen_golden_strcmp.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in C.CASES:
        try:
            out = G.run(case, table)
        except Exception as exc:      # the reference raises on this shape: no fixture, the pyarrow-based tests carry it
            meta["dropped"][case["name"]] = f"{type(exc).__name__}: {exc}"[:300]
            print(f"{case['name']:20s} DROPPED  {type(exc).__name__}: {exc}")
            continue
        write(f"strcmp_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:20s} {out.num_rows:6d} rows  {out.schema.names}")
    with open(os.path.join(HERE, "strcmp_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
