#!/usr/bin/env python3
"""Outputs of the REAL reference aggregate (oracle/_ref/libvinum_ref.so: the reference's own C++ operators; build container
only) on the seeded tables of live_cases.py, for tests/test_oracle_golden.py::test_oracle_matches_live_reference to compare
the oracle with where oracle/_ref is not built.

  live_ref_s<seed>_k<kind>.arrow   one file per seed and aggregate kind (SINGLE / MULTI / ONE_GROUP)
  live_cases.json                  SHA-256 of every input table (float_cases.table_digest)

Usage:  python tests/golden/gen_golden_live.py          (from the repo root)
"""
import json
import os
import sys

import numpy as np
import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref  # noqa: E402
from tests.golden import float_cases as F  # noqa: E402
from tests.golden import live_cases as C  # noqa: E402


def write(name, table):
    with pa.OSFile(os.path.join(HERE, name), "wb") as f:
        with pa.ipc.new_file(f, table.schema) as w:
            w.write_table(table)


def main():
    digests = {}
    for seed in C.SEEDS:
        t = C.table(seed)
        digests[str(seed)] = F.table_digest(t)
        for kind, gb in C.KINDS:
            agg = ref.RefAggregate(kind, gb, gb, C.FUNCS)
            tc = t.combine_chunks()
            for start in range(0, tc.num_rows, C.CHUNK):
                for b in tc.slice(start, C.CHUNK).to_batches():
                    agg.next(b)
            write(C.golden_name(seed, kind), pa.Table.from_batches([agg.result()]))
    with open(os.path.join(HERE, "live_cases.json"), "w") as f:
        json.dump({"sha256": digests, "numpy": np.__version__,
                   "generator": "tests/golden/gen_golden_live.py over oracle/_ref (the reference's own aggregate)"}, f, indent=1)


if __name__ == "__main__":
    assert ref.available(), "build oracle/_ref first: make -C oracle/ref_build"
    main()
