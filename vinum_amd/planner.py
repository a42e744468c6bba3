"""Query planner for the GPU operators: the build's counterpart of QueryPlanner.plan_query
(vinum/planner/planner.py:330-507) for queries given as data instead of SQL text (the reference parses SQL with pglast,
which is out of scope -- SURVEY.md §2; its own tests feed Query ASTs of exactly this content).

    reader -> [Filter] -> [Project inner aggregate / group-by expressions, keep_input] -> [Aggregate] -> [Filter HAVING]
           -> [Sort] -> Project(select list) -> [Slice] -> Materialize                      (planner.py:360-505)

A query is a dict (see tests/golden/planner_cases.py):
    select     [expr]            aliases [str | None]      distinct bool
    where      expr | None       group_by [expr]           having expr | None
    order_by   [expr]            sort_order ["ASC" | "DESC"]   limit int | None   offset int
    expr := the prefix tuples of vinum_amd.expr (the one definition of the node forms), with ("fn", name, arg...) for the
            aggregate functions count_star / count / sum / avg / min / max and the numeric built-in scalar functions
            (SCALAR_FN_NAMES: abs, sqrt, sin, ..., to_int, pi, e and their np. spellings), upper / lower of a string
            column, to_str of an integer, date32, timestamp or string column and date / datetime / from_timestamp (the unit a
            ("lit", unit) argument) of a string, date32 / timestamp or -- from_timestamp -- integer column, which are per-row expressions; concat is the operator node ("concat", x, ...) or ("||", a, b) over string
            columns, such nodes, upper / lower and literals (("lit", s), numbers), and they are per-row expressions wherever they appear, like any operator; LIKE / NOT LIKE against a utf8 / large_utf8 column (planner.py:189-193)
            may stand in WHERE, HAVING, the SELECT list (a uint8 mask) and aggregate arguments alike.

What the planner does with the aggregate part mirrors planner.py:380-469:
  * DISTINCT = GROUP BY every select expression (:380-382);
  * an aggregate over an EXPRESSION (`sum((1 - total) * (2 + tax))`, test_query_results.py:436-443) and a GROUP BY
    expression become columns of a pre-aggregate projection that keeps the input (:384-417);
  * every aggregate function node -- in SELECT, HAVING or ORDER BY -- becomes one function of the AggregateOperator and is
    replaced by its output column in the post-aggregate expressions (:419-448), so HAVING is a filter and
    `sum(a) / count(*)` a projection over the G-row result.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import pyarrow as pa

from .core import (AggregateFunction, AggregateOperator, FileReaderOperator, FilterOperator, MaterializeTableOperator,
                   ProjectOperator, SliceOperator, SortOperator, TableReaderOperator)
from . import expr as E
from .expr import columns_of
from .core.lowering import check_temporal
from .keydict import device_value_type, temporal_operand_kind, to_str_kind

AGG_FUNCS = ("count_star", "count", "sum", "avg", "min", "max")     # vinum/core/functions.py:389-396
# numeric part of _default_functions_registry (vinum/core/functions.py:353-387) and the `np.` spellings lookup_udf resolves
# to the same ufuncs (vinum/core/udf.py:28-64) -> the vinum_amd.ops operator name
SCALAR_FN_NAMES = {n: n for n in ("abs", "sqrt", "cos", "sin", "tan", "power", "log", "log2", "log10", "to_int", "to_float",
                                  "to_bool", "pi", "e")}
SCALAR_FN_NAMES.update({"np." + n: n for n in ("sqrt", "cos", "sin", "tan", "power", "log", "log2", "log10", "abs")})
SCALAR_FN_NAMES["np.absolute"] = "abs"
# the string built-ins that run on the device: a function of the column's dictionary (core.lowering.lower_case_functions)
SCALAR_FN_NAMES.update({"upper": "upper", "lower": "lower"})
# to_str (StringCastFunction, functions.py:189-193, 'to_str' at :358): a function of the column's VALUE (keydict.ValueTable)
SCALAR_FN_NAMES["to_str"] = "to_str"
# the datetime built-ins (functions.py:25-137, registered at :376-379): over a string column a function of the dictionary's values
# (KeyDictionary.parsed_column), over a temporal column a change of unit, over literals a constant folded by NumPy
SCALAR_FN_NAMES.update({n: n for n in E.TEMPORAL_FNS})
# the rest of the datetime family (functions.py:380-381, :375): timedelta folds into a constant, now() folds ONCE per query (plan_query),
# is_busday is a mask kernel; arithmetic over temporal values is typed by core.lowering.TemporalArithmetic
SCALAR_FN_NAMES.update({"timedelta": "timedelta", "is_busday": "is_busday", "now": "now"})


def _t(e):
    """JSON lists -> tuples (hashable, and what ops.compile_expr takes); IN value lists stay lists.  A built-in scalar
    function ("fn", "sqrt", x) becomes the operator node ("sqrt", x); aggregate and unknown names stay "fn" nodes.  concat is written
    as the operator node it is -- ("concat", a, ("lit", "-"), 7, b) or ("||", a, b), literals as they are --; the "fn" spelling of
    that name stays the unknown function it has always been to this planner."""
    if isinstance(e, (list, tuple)) and e and isinstance(e[0], str):
        if e[0] in E.IN_OPS:                                  # (a member may be a date() / datetime() node: a temporal constant)
            return (e[0], _t(e[1]), tuple(_t(v) if isinstance(v, (list, tuple)) else v for v in e[2]))
        if e[0] == "fn" and len(e) > 1 and isinstance(e[1], str) and e[1].lower() in SCALAR_FN_NAMES:
            e = [SCALAR_FN_NAMES[e[1].lower()]] + list(e[2:])
        if e[0] == "is_busday" and len(e) > 3 and isinstance(e[3], (list, tuple)) and not E.is_str_lit(tuple(e[3])):
            # the holidays are a list literal of date strings, no operand: kept as a tuple of plain strings
            days = tuple(h[1] if isinstance(h, (list, tuple)) and len(h) == 2 and h[0] == "lit" else h for h in e[3])
            return tuple([e[0]] + [_t(x) for x in e[1:3]]) + (days,) + tuple(_t(x) for x in e[4:])
        if e[0] == "||":                                      # SQLExpression.CONCAT: the same function as concat()
            return tuple(["concat"] + [_t(x) for x in e[1:]])
        return tuple([e[0]] + [_t(x) for x in e[1:]])
    return e


def _case_by_type(e, schema):
    """upper(x) / lower(x) are the string built-ins where x can be a string.  Over a NUMERIC column of a table -- whose schema is
    known at plan time -- the name is no function of this planner, and the query is refused as one with any unknown function is
    ("unknown aggregate function 'upper'"; the reference would print the numbers as text, which is not restated).  Without a schema
    (a file source, the adapter) the lowering raises TypeError for such an operand when the batch arrives (core.lowering)."""
    # arithmetic over temporal values, timedelta(), is_busday() and IN lists of temporal constants: the lowering's own type rules over
    # the schema (core.lowering.check_temporal) accept what runs and refuse here what a batch would be refused for
    if e is not None and any(isinstance(n, tuple) and n and (n[0] in ("timedelta", "is_busday") or n[0] in E.TEMPORAL_ARITH or n[0] in E.IN_OPS)
                             for n in E.nodes(e)):
        check_temporal(e, {f.name: f.type for f in schema})
    for n in E.nodes(e) if e is not None else ():
        if isinstance(n, tuple) and n and n[0] in ("upper", "lower") and len(n) == 2 and isinstance(n[1], str) and n[1] in schema.names:
            t = schema.field(n[1]).type
            if pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_temporal(t):
                raise ValueError(f"unknown aggregate function {n[0]!r}: upper() / lower() take a string column, {n[1]!r} is {t}")
        # to_str(x): the types without a formatter on the device (floats, decimal, date64, time, duration, boolean, binary) are refused
        # here, naming the column (keydict.to_str_kind); an operand that is no column is refused by the lowering
        if isinstance(n, tuple) and n and n[0] == "to_str" and len(n) == 2 and isinstance(n[1], str) and n[1] in schema.names:
            t = schema.field(n[1]).type
            dt = device_value_type(t)
            if dt is None or pa.types.is_binary(dt) or pa.types.is_large_binary(dt):
                to_str_kind(t, n[1])
        # date(x) / datetime(x[, unit]) / from_timestamp(x[, unit]): the unit against the function's list (ValueError, the reference's
        # message), a literal operand folded once to surface NumPy's parse error, a column's type against what the function takes
        if isinstance(n, tuple) and n and n[0] in E.TEMPORAL_FNS:
            E.temporal_unit_arg(n)
            if E.fold_temporal(n) is None and isinstance(n[1], str) and n[1] in schema.names:
                temporal_operand_kind(n[0], schema.field(n[1]).type, n[1])
        # concat(x, ...): a BARE numeric or temporal column stays refused here, by name -- the explicit spelling is concat(to_str(x), ...)
        if isinstance(n, tuple) and n and n[0] == "concat":
            for x in n[1:]:
                if isinstance(x, str) and x in schema.names:
                    t = schema.field(x).type
                    if pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_temporal(t) or pa.types.is_boolean(t) or pa.types.is_decimal(t):
                        raise TypeError(f"concat() needs string columns and literals, {x!r} is {t} (write to_str({x}) for its text)")


def _is_fn(e) -> bool:
    return isinstance(e, tuple) and e[0] == "fn"


def _has_fn(e) -> bool:
    return any(_is_fn(n) for n in E.nodes(e))


def output_names(select: Sequence, aliases: Sequence[Optional[str]]) -> List[str]:
    """QueryPlanner._column_names (planner.py:299-328): alias, else the column / function name, else col_<n>; a repeated
    name gets _<k>."""
    names, seen, unnamed = [], {}, 0
    for e, a in zip(select, aliases):
        if a:
            name = a
        elif isinstance(e, str):
            name = e
        elif _is_fn(e):
            name = e[1]
        else:
            name = f"col_{unnamed}"
            unnamed += 1
        if name in seen:
            seen[name] += 1
            name = f"{name}_{seen[name]}"
        else:
            seen[name] = 0
        names.append(name)
    return names


class Plan:
    """The operator chain plus what was decided on the way (tests compare it with the reference's plan shape)."""

    def __init__(self, root, steps):
        self.root, self.steps = root, steps

    def execute(self) -> pa.Table:
        return next(self.root.next())


def plan_query(query: Dict, source, expected_groups: int = 0) -> Plan:
    select = [_t(e) for e in query["select"]]
    aliases = list(query.get("aliases") or [None] * len(select))
    where = _t(query.get("where"))
    group_by = [_t(e) for e in query.get("group_by") or []]
    having = _t(query.get("having"))
    order_by = [_t(e) for e in query.get("order_by") or []]
    sort_order = [1 if str(s).upper().endswith("DESC") else 0 for s in (query.get("sort_order") or ["ASC"] * len(order_by))]
    limit, offset = query.get("limit"), query.get("offset") or 0
    distinct = bool(query.get("distinct"))
    steps = []
    # now() folds ONCE per query: every occurrence, in every clause, is the same instant (expr.fold_now)
    n_sel, n_grp = len(select), len(group_by)
    folded = E.fold_now(select + group_by + order_by + [where, having])
    select, group_by, order_by = folded[:n_sel], folded[n_sel:n_sel + n_grp], folded[n_sel + n_grp:-2]
    where, having = folded[-2:]
    if isinstance(source, pa.Table):
        for e in select + group_by + order_by + [where, having]:
            _case_by_type(e, source.schema)

    # ---- column pruning (planner.py:346-371): only what the query touches is staged into HBM
    used: List[str] = []
    for e in select + ([where] if where is not None else []) + group_by + ([having] if having is not None else []) + order_by:
        for c in columns_of(e):
            if c not in used:
                used.append(c)
    if isinstance(source, pa.Table):
        if not used and source.num_columns:
            used = [source.schema.names[0]]          # count(*) only: keep one column for the row count (:354-355)
        op = TableReaderOperator(source, columns=used)
    else:
        if hasattr(source, "read_next_device_batch") and used:
            source._want = [c for c in used]          # column pruning reaches the CSV parser: only these fields are parsed
        op = FileReaderOperator(source, columns=used or None)
    steps.append(("read", tuple(used)))

    if where is not None:
        pred = _simple_predicate(where)
        op = FilterOperator(pred if pred is not None else where, op)
        steps.append(("filter", where))

    is_agg = distinct or bool(group_by) or any(_has_fn(e) for e in select)
    if distinct:
        group_by = group_by + [e for e in select if e not in group_by]      # planner.py:380-382
    if is_agg:
        inner: Dict[Tuple, str] = {}      # expression -> pre-aggregate column

        def inner_col(e):
            if isinstance(e, str):
                return e
            if e not in inner:
                inner[e] = f"__inner_{len(inner)}"
            return inner[e]

        # aggregate function nodes -> functions of the operator (one per distinct (function, input)).  An argument that is
        # an EXPRESSION stays an expression: the aggregate operator hands it to the kernel (evaluated in registers in the
        # hot shape) or projects it itself -- the reference plans a keep-input projection for it (planner.py:384-417)
        funcs: Dict[Tuple[str, object], str] = {}
        key_of_expr: Dict[Tuple, str] = {}

        def fn_col(node):
            if not _is_fn(node):
                return node
            name = node[1].lower()
            if name not in AGG_FUNCS:
                raise ValueError(f"unknown aggregate function {node[1]!r}")
            arg = node[2] if len(node) > 2 and not isinstance(node[2], (int, float)) else ""
            if isinstance(arg, tuple) and arg in key_of_expr:
                arg = key_of_expr[arg]                    # the argument is a GROUP BY expression: already a column
            if name == "count" and not arg:
                name = "count_star"
            key = (name, arg)
            if key not in funcs:
                funcs[key] = f"__agg_{len(funcs)}"
            return funcs[key]

        key_cols = [inner_col(e) for e in group_by]
        key_of = dict(zip(group_by, key_cols))
        key_of_expr.update({e: c for e, c in key_of.items() if isinstance(e, tuple)})

        def post(e):
            """an expression over the aggregate's OUTPUT: functions and group-by expressions become columns"""
            if e in key_of:
                return key_of[e]
            return E.transform(e, lambda n: key_of.get(n, fn_col(n)))

        select_post = [post(e) for e in select]
        having_post = post(having) if having is not None else None
        order_post = [post(e) for e in order_by]
        if inner:
            op = ProjectOperator(list(inner.keys()), op, col_names=list(inner.values()), keep_input_table=True)
            steps.append(("project_inner", tuple(inner.items())))
        agg_funcs = [AggregateFunction(f, (arg or None) if isinstance(arg, str) else None, out, expr=arg if isinstance(arg, tuple) else None)
                     for (f, arg), out in funcs.items()]
        op = AggregateOperator(op, key_cols, agg_funcs, key_cols, expected_groups=expected_groups)
        steps.append(("aggregate", tuple(key_cols), tuple(funcs.items())))
        select, having, order_by = select_post, having_post, order_post
        if having is not None:
            pred = _simple_predicate(having)
            op = FilterOperator(pred if pred is not None else having, op)
            steps.append(("having", having))

    names = output_names([_raw(e) for e in query["select"]], aliases)
    if order_by:
        # ORDER BY expressions are evaluated into extra columns, sorted by, and dropped by the final projection
        # (SortOperator.next, algebra.py:159-177)
        sort_cols, extra = [], {}
        for e in order_by:
            if isinstance(e, str):
                sort_cols.append(e)
            else:
                extra.setdefault(e, f"__sort_{len(extra)}")
                sort_cols.append(extra[e])
        if extra:
            op = ProjectOperator(list(extra.keys()), op, col_names=list(extra.values()), keep_input_table=True)
        push = (limit + offset) if limit is not None else 0
        op = SortOperator(sort_cols, sort_order, op, limit=push)
        steps.append(("sort", tuple(sort_cols), tuple(sort_order)))
    op = ProjectOperator(select, op, col_names=names)
    steps.append(("project", tuple(select), tuple(names)))
    if limit is not None:
        op = SliceOperator(limit, offset, op)
        steps.append(("slice", limit, offset))
    return Plan(MaterializeTableOperator(op), steps)


def _raw(e):
    """the select expression as written (a function keeps its "fn" node: the reference names the column after it)"""
    if isinstance(e, (list, tuple)) and e and e[0] == "fn":
        return tuple(e)
    return _t(e)


def execute(query: Dict, source, expected_groups: int = 0) -> pa.Table:
    return plan_query(query, source, expected_groups).execute()


def _simple_predicate(e):
    """`column <op> literal` -> the (column, op, literal) triple FilterOperator fuses (vnm_filter_cmp / the aggregate scan)"""
    if (isinstance(e, tuple) and len(e) == 3 and e[0] in E.CMP_SYMBOL and isinstance(e[1], str)
            and isinstance(e[2], (int, float)) and not isinstance(e[2], bool)):
        return (e[1], E.CMP_SYMBOL[e[0]], e[2])
    return None
