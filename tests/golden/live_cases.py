"""Seeded inputs of the oracle-vs-reference aggregate cases (pure NumPy: no reference code).

Shared by tests/golden/gen_golden_live.py (which runs the REAL reference over them in the build container and commits its
outputs, live_ref_s<seed>_k<kind>.arrow, plus a SHA-256 of every input table in live_cases.json) and by
tests/test_oracle_golden.py, which regenerates the same inputs from the seeds and refuses to compare if a checksum differs.
"""
import numpy as np
import pyarrow as pa

COUNT_STAR, COUNT, MIN, MAX, SUM, AVG = range(6)
ONE_GROUP, SINGLE, MULTI = range(3)

SEEDS = [0, 1, 2]
CHUNK = 3000
FUNCS = [(COUNT_STAR, "", "n"), (COUNT, "v", "cv"), (SUM, "v", "sv"), (AVG, "v", "av"),
         (MIN, "v", "mnv"), (MAX, "v", "mxv"), (SUM, "w", "sw"), (AVG, "w", "aw")]
KINDS = [(SINGLE, ["k"]), (MULTI, ["k", "k2"]), (ONE_GROUP, [])]


def table(seed) -> pa.Table:
    """NULL keys and values, lognormal floats and int64 values near +-2^62 (64-bit sums overflow into the wide path)."""
    rng = np.random.default_rng(100 + seed)
    n = 20000
    return pa.table({
        "k": pa.array(rng.integers(-50, 50, n).astype(np.int64), mask=rng.random(n) < 0.02),
        "k2": pa.array(rng.integers(0, 5, n).astype(np.int16), mask=rng.random(n) < 0.02),
        "v": pa.array(rng.lognormal(2, 1, n), mask=rng.random(n) < 0.1),
        "w": pa.array(rng.integers(-2**62, 2**62, n).astype(np.int64), mask=rng.random(n) < 0.1),
    })


def golden_name(seed, kind) -> str:
    return f"live_ref_s{seed}_k{kind}.arrow"
