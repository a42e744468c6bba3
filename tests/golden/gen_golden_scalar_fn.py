#!/usr/bin/env python3
"""Fixtures for the built-in scalar functions from the reference's OWN planner + executor (build container only).

Reuses to_ast / run of gen_golden_planner.py (same stubs: oracle/pglast_stub for the absent pglast, oracle/ref_vinum_lib
over the reference operators built into oracle/_ref).  One adjustment: that generator decides Query.is_aggregate with a
`has_agg` that counts every function node, which was right while only aggregates were functions.  The reference's
parser asks is_aggregate_func (vinum/core/functions.py:409-423), so it is replaced here by the same test -- without editing
the other generator.

Outputs (data only): scalarfn_<name>.arrow = the reference's result of tests/golden/scalar_fn_cases.CASES over
scalar_fn_table() (regenerated from its seed, SHA-256 in scalarfn_cases.json).  The float16 results of sqrt / sin / ...
over 8-bit integers travel through the whole query (case "float16"), so no case needs an expression-level record.

Usage:  PYTHONPATH=oracle/pglast_stub:/root/reference python -B tests/golden/gen_golden_scalar_fn.py
"""
import json
import os
import sys
import warnings

import numpy as np
import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import gen_golden_planner as G  # noqa: E402  (sets up the reference import path and stubs)
from tests.golden import scalar_fn_cases as S  # noqa: E402
from tests.golden.float_cases import table_digest  # noqa: E402
import vinum  # noqa: E402
from vinum.core.functions import is_aggregate_func  # noqa: E402


def has_agg(e):
    return isinstance(e, list) and ((e[0] == "fn" and bool(is_aggregate_func(e[1])))
                                    or any(has_agg(a) for a in e[1:]))


G.has_agg = has_agg


def write(name, table):
    with pa.OSFile(os.path.join(HERE, name), "wb") as f:
        with pa.ipc.new_file(f, table.schema) as w:
            w.write_table(table.combine_chunks())


def main():
    warnings.simplefilter("ignore")
    vinum.set_batch_size(6000)
    table = S.scalar_fn_table()
    meta = {"table_sha256": table_digest(table), "cases": {}, "pyarrow": pa.__version__, "numpy": np.__version__,
            "generator": "tests/golden/gen_golden_scalar_fn.py: the reference's QueryPlanner + RecursiveExecutor"}
    for case in S.CASES:
        with np.errstate(all="ignore"):
            out = G.run(case, table)
        write(f"scalarfn_{case['name']}.arrow", out)
        meta["cases"][case["name"]] = {"rows": out.num_rows, "columns": out.schema.names, "types": [str(t) for t in out.schema.types]}
        print(f"{case['name']:20s} {out.num_rows:6d} rows  {out.schema.names}")
    with open(os.path.join(HERE, "scalarfn_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
