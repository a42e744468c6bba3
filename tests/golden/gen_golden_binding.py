#!/usr/bin/env python3
"""What the reference's UNCHANGED planner builds with vinum_amd.binding.install() applied, for every query of
tests/golden/planner_cases.py -> binding_ref.json (build container only: needs the reference sources and oracle/_ref).
tests/test_binding_cpu.py compares what vinum_amd's own planner derives with it.

  lowered  {case: [repr of binding.lower(tree)]}: the SELECT / WHERE expressions as VectorizedExpression trees over the
           reference's own classes and registry callables, lowered to the programs the GPU kernels execute
  plans    {case: {...}}: the programs held by the GPU Filter / Project operators of the reference's plan

Usage:  VNM_REFERENCE_DIR=<reference checkout> python -B tests/golden/gen_golden_binding.py      (from the repo root)
"""
import contextlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import planner_cases as P  # noqa: E402

OUT = os.path.join(HERE, "binding_ref.json")


def available(ref_dir) -> bool:
    return bool(ref_dir) and os.path.isdir(os.path.join(ref_dir, "vinum")) and \
        os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libvinum_ref.so"))


@contextlib.contextmanager
def reference(ref_dir):
    """The reference's `vinum` package importable, its `vinum_lib` bound to the reference operators in oracle/_ref."""
    stub = os.path.join(ROOT, "oracle", "pglast_stub")
    sys.path.insert(0, stub)
    sys.path.append(ref_dir)
    old = sys.dont_write_bytecode
    sys.dont_write_bytecode = True           # the reference checkout stays untouched
    try:
        from oracle import ref_vinum_lib
        sys.modules["vinum_lib"] = ref_vinum_lib
        import vinum
        from tests.golden import gen_golden_planner as G
        yield vinum, G
    finally:
        sys.dont_write_bytecode = old
        for m in [k for k in sys.modules if k == "vinum" or k.startswith("vinum.") or k in ("vinum_lib", "pglast", "pglast.enums")]:
            del sys.modules[m]
        sys.path.remove(ref_dir)
        sys.path.remove(stub)


def norm(e):
    if isinstance(e, tuple) and e and e[0] in ("in", "not_in"):
        return (e[0], norm(e[1]), tuple(e[2]))
    if isinstance(e, tuple):
        return tuple([e[0]] + [norm(x) for x in e[1:]])
    return e


def shape(e):
    """expression with column names that are planner-internal ids replaced by '#' (aggregate outputs, shared ids)"""
    if isinstance(e, str):
        return "#" if (e.startswith("__") or any(ch.isdigit() for ch in e) and ("_" in e)) else e
    if isinstance(e, tuple):
        if e[0] in ("in", "not_in"):
            return (e[0], shape(e[1]), tuple(e[2]))
        return tuple([e[0]] + [shape(x) for x in e[1:]])
    return e


def case_exprs(case):
    """The SELECT / WHERE expressions of a case that lower to a program of their own."""
    from vinum_amd import binding as B
    from vinum_amd.planner import _t
    out = []
    for e in case["select"] + ([case["where"]] if case["where"] is not None else []):
        e = _t(e)
        if isinstance(e, tuple) and not B.ops.columns_of(e) and e[0] != "fn":
            continue
        if isinstance(e, tuple) and e[0] == "fn" and len(e) > 2 and not isinstance(e[2], str):
            continue     # aggregate over an expression: the planner replaces the argument by a column first
        out.append(e)
    return out


def lowered(vinum):
    from vinum.core import expressions as E
    from vinum.core.base import VectorizedExpression as VE
    from vinum.core.aggregate import AggregateFunction as AF
    from vinum.core.functions import FunctionType as FT
    from vinum.parser.query import Column, Literal, SQLExpression
    from vinum_amd import binding as B
    index = B.registry_index(E.EXPRESSION_FUNCTIONS)
    classes = (Column, Literal, VE, AF, SQLExpression, FT, E.BINARY_EXPRESSIONS)
    return {case["name"]: [repr(B.lower(B.vectorize(e, registry=E.EXPRESSION_FUNCTIONS, classes=classes), index))
                           for e in case_exprs(case)] for case in P.CASES}


def _chain(op):
    out = []
    while op is not None:
        out.append(op)
        op = getattr(op, "_parent_operator", None)
    return out[::-1]


def plan_record(case, vinum, G):
    from vinum.arrow.arrow_table import ArrowTable
    from vinum.parser.query import Query, SortOrder
    from vinum.planner import planner as RP
    from vinum_amd import binding as B
    table = P.TABLES[case.get("table", "main")]()
    saved = (RP.FilterOperator, RP.ProjectOperator)
    try:
        B.install(vinum)
        sel = tuple(G.to_ast(e, a) for e, a in zip(case["select"], case["aliases"]))
        is_agg = bool(case["group_by"]) or any(G.has_agg(e) for e in case["select"])
        q = Query(table.schema, sel, is_agg, case["distinct"],
                  G.to_ast(case["where"]) if case["where"] is not None else None,
                  tuple(G.to_ast(e) for e in case["group_by"]),
                  G.to_ast(case["having"]) if case["having"] is not None else None,
                  tuple(G.to_ast(e) for e in case["order_by"]),
                  tuple(SortOrder[s] for s in case["sort_order"]), case["limit"], case["offset"])
        plan = RP.QueryPlanner(q, table=ArrowTable(table)).plan_query()
    finally:
        RP.FilterOperator, RP.ProjectOperator = saved
    ops_ref = _chain(plan)
    filters = [o for o in ops_ref if isinstance(o, B.GpuFilterOperator)]
    projects = [o for o in ops_ref if isinstance(o, B.GpuProjectOperator)]
    inner = [p for p in projects[:-1] if p._inner._keep]
    return {"n_filters": len(filters),
            "where": repr(filters[0].predicate) if case["where"] is not None and filters else None,
            "having": repr(shape(filters[-1].predicate)) if case["having"] is not None and filters else None,
            "final_cols": list(projects[-1]._inner._col_names),
            "final": [repr(shape(e)) for e in projects[-1].expressions],
            "inner": sorted(map(repr, (norm(e) for e in inner[-1].expressions))) if inner else None}


def records(vinum, G):
    return {"lowered": lowered(vinum), "plans": {case["name"]: plan_record(case, vinum, G) for case in P.CASES}}


def main():
    ref_dir = os.environ.get("VNM_REFERENCE_DIR", "")
    assert available(ref_dir), "set VNM_REFERENCE_DIR to the reference sources and build oracle/_ref (make -C oracle/ref_build)"
    with reference(ref_dir) as (vinum, G):
        rec = records(vinum, G)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
