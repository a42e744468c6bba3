"""Built-in scalar functions in whole queries vs fixtures produced by the reference's OWN planner + executor.

tests/golden/scalarfn_<case>.arrow were written by tests/golden/gen_golden_scalar_fn.py (the reference's QueryPlanner +
RecursiveExecutor over tests/golden/scalar_fn_cases.py).  Every case runs through vinum_amd.planner; the filter /
projection cases also run through the B2 adapter (GpuFilterOperator / GpuProjectOperator over VectorizedExpression trees
built with the mirror classes, the way the installed planner builds them).

Comparison: exact columns bit for bit (NaN as a class: the NaN an invalid operation creates is the host's default NaN
in the fixture, the canonical NaN on the GPU), derived integer keys exactly; transcendental columns within 6 ULP of the
fixture (NumPy evaluates them with SVML on x86, up to 4 ULP; the GPU is within 2-3 ULP of the correctly rounded value);
float SUM / AVG follow DESIGN.md §2 (the correctly rounded sum, not the reference's sequential one): relative 1e-12."""
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from tests import util
from tests.golden import scalar_fn_cases as S
from tests.golden.float_cases import table_digest

pytestmark = pytest.mark.gpu

AGG_FLOAT = {("agg_sqrt_power", "s"), ("agg_sqrt_power", "p")}
SORT_KEYS = {"why_groupby": ["city_from", "grp_exp"], "agg_sqrt_power": ["k"], "having_to_float": ["k"]}


@pytest.fixture(scope="module")
def table():
    t = S.scalar_fn_table()
    with open(os.path.join(util.GOLDEN, "scalarfn_cases.json")) as f:
        meta = json.load(f)
    assert table_digest(t) == meta["table_sha256"], "NumPy produced a different input table than the generator saw"
    return t


def _ordered(t: pa.Table, case) -> pa.Table:
    keys = SORT_KEYS.get(case["name"])
    return t.sort_by([(k, "ascending") for k in keys]) if keys else t


def _col_equal(g: np.ndarray, e: np.ndarray, what, approx, agg):
    assert g.dtype == e.dtype, (what, g.dtype, e.dtype)
    if e.dtype.kind != "f":
        assert np.array_equal(g, e), (what, np.flatnonzero(g != e)[:5])
        return
    gn, en = np.isnan(g), np.isnan(e)
    assert np.array_equal(gn, en), (what, np.flatnonzero(gn != en)[:5])
    g, e = g[~gn], e[~en]
    inf = ~np.isfinite(e)
    assert np.array_equal(g[inf], e[inf]), what
    g, e = g[~inf], e[~inf]
    if agg:
        assert np.allclose(g, e, rtol=1e-12, atol=0), what
    elif approx:
        spacing = np.abs(np.spacing(e)).astype(np.float64)
        ulps = np.abs(g.astype(np.float64) - e.astype(np.float64)) / spacing
        assert ulps.max(initial=0) <= 6, (what, ulps.max())
        assert np.array_equal(np.signbit(g[e == 0]), np.signbit(e[e == 0])), what
    else:
        w = f"u{e.dtype.itemsize}"
        bad = g.view(w) != e.view(w)
        assert not bad.any(), (what, g[bad][:5], e[bad][:5])


def _compare(got: pa.Table, exp: pa.Table, case):
    assert got.schema.names == exp.schema.names, (case["name"], got.schema.names, exp.schema.names)
    assert got.num_rows == exp.num_rows, (case["name"], got.num_rows, exp.num_rows)
    got, exp = _ordered(got.combine_chunks(), case), _ordered(exp.combine_chunks(), case)
    for name in exp.schema.names:
        g = got.column(name).to_numpy(zero_copy_only=False)
        e = exp.column(name).to_numpy(zero_copy_only=False)
        _col_equal(g, e, f"{case['name']}.{name}", name in case["approx"], (case["name"], name) in AGG_FLOAT)


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c["name"])
def test_scalarfn_golden_through_the_planner(case, table):
    from vinum_amd import planner, set_batch_size
    set_batch_size(1500)          # several batches per query
    try:
        got = planner.execute(case, table)
    finally:
        set_batch_size(1 << 24)
    _compare(got, util.read_ipc(f"scalarfn_{case['name']}.arrow"), case)


@pytest.mark.parametrize("case", [c for c in S.CASES if not c["group_by"] and not c["order_by"]
                                  and not any(isinstance(e, list) and e[:2] in (["fn", "sum"], ["fn", "avg"]) for e in c["select"])],
                         ids=lambda c: c["name"])
def test_scalarfn_golden_through_the_b2_adapter(case, table):
    from vinum_amd import binding as B
    from vinum_amd.core import MaterializeTableOperator, TableReaderOperator
    from vinum_amd.planner import _raw, _t, output_names
    op = TableReaderOperator(table)
    if case["where"] is not None:
        op = B.GpuFilterOperator(B.vectorize(_t(case["where"])), op)
    sel = [_t(e) for e in case["select"]]
    op = B.GpuProjectOperator([B.vectorize(e) for e in sel], op,
                              col_names=output_names([_raw(e) for e in case["select"]], case["aliases"]))
    got = next(MaterializeTableOperator(op).next())
    _compare(got, util.read_ipc(f"scalarfn_{case['name']}.arrow"), case)
