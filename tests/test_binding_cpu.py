"""Seam B2 on the CPU: the adapter consumes what the reference's UNCHANGED planner builds.

The reference's QueryPlanner plans every query of tests/golden/planner_cases.py with vinum_amd.binding.install() applied
(which only rebinds the FilterOperator / ProjectOperator names in the planner's namespace).  The GPU operators it then
instantiates must hold exactly the expressions vinum_amd's own planner derives from the same query, i.e. the
VectorizedExpression trees carrying the reference's registry callables lower to the programs the GPU tests execute.
The reference side is stored in tests/golden/binding_ref.json (tests/golden/gen_golden_binding.py); where
VNM_REFERENCE_DIR names the reference sources and oracle/_ref is built, it is also computed live and must equal the stored
record.  No GPU is touched."""
import json
import os

import pytest

from tests.golden import gen_golden_binding as GB
from tests.golden import planner_cases as P

with open(GB.OUT) as _f:
    STORED = json.load(_f)


@pytest.fixture(scope="module")
def ref_env():
    ref_dir = os.environ.get("VNM_REFERENCE_DIR", "")
    if not GB.available(ref_dir):
        yield None
        return
    with GB.reference(ref_dir) as env:
        yield env


def test_lower_reads_the_reference_registry(ref_env):
    from vinum_amd import binding as B
    ref = STORED["lowered"]
    if ref_env is not None:
        assert GB.lowered(ref_env[0]) == ref, "binding_ref.json is out of date: run tests/golden/gen_golden_binding.py"
    for case in P.CASES:
        exprs = GB.case_exprs(case)
        assert len(ref[case["name"]]) == len(exprs), case["name"]
        for got, e in zip(ref[case["name"]], exprs):
            assert got == repr(B.lower(B.vectorize(e))) == repr(GB.norm(e)), case["name"]


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c["name"])
def test_installed_operators_hold_the_programs_our_planner_derives(case, ref_env):
    from vinum_amd import planner as OP
    rec = STORED["plans"][case["name"]]
    if ref_env is not None:
        assert GB.plan_record(case, *ref_env) == rec, "binding_ref.json is out of date: run tests/golden/gen_golden_binding.py"
    table = P.TABLES[case.get("table", "main")]()
    steps = dict((s[0], s) for s in OP.plan_query(case, table).steps)
    # WHERE / HAVING: same predicate program (modulo the internal names of aggregate output columns)
    n_filters = (case["where"] is not None) + (case["having"] is not None)
    assert rec["n_filters"] == n_filters
    if case["where"] is not None:
        assert rec["where"] == repr(GB.norm(OP._t(case["where"]))), "WHERE lowered differently"
    if case["having"] is not None:
        assert rec["having"] == repr(GB.shape(steps["having"][1])), "HAVING lowered differently"
    # the final projection: same expressions up to the names of intermediate columns, same output names
    assert rec["final_cols"] == list(steps["project"][2])
    assert rec["final"] == [repr(GB.shape(e)) for e in steps["project"][1]]
    # expressions inside aggregates / GROUP BY expressions: one keep-input projection holding the same expressions
    # (our planner keeps an aggregate ARGUMENT expression inside the aggregate function -- the kernel evaluates it -- and
    # only projects GROUP BY expressions; the reference projects both: the union must be the same set of expressions)
    ours = [e for e, _ in steps["project_inner"][1]] if "project_inner" in steps else []
    if "aggregate" in steps:
        ours += [arg for (_f, arg), _out in steps["aggregate"][2] if isinstance(arg, tuple)]
    if ours:
        assert rec["inner"] is not None, "the reference plan has no pre-aggregate projection"
        assert rec["inner"] == sorted(repr(e) for e in ours)
