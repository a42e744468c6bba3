"""The expression tree of the GPU operators: its grammar, its walkers and the passes that need nothing but the tree.

An expression is a nested prefix tuple.  This docstring is the one written definition of the node forms, and _OPERANDS below the one
table of where a form keeps its sub-expressions: operands(), with_operands() and the walkers read it, a pass reads the walkers:

    "name"                          a column (a bare str is ALWAYS a column name)
    1, 2.5                          a number: a weak Python literal, typed by the operand it meets (NumPy 2 rules); bool is none
    ("strong", v)                   a number with an array's strong type (int64 / float64): what fold() and an IN list produce
    ("lit", v)                      a string / bytes literal -- `city = 'Berlin'`, a LIKE pattern
    (op, x[, y...])                 an operator of ops._EX or a comparison (CMP_SYMBOLS, by symbol or by name); n-ary chains fold
                                    left like VectorizedExpression._apply_binary_args_function (vinum/core/base.py:145-151)
    ("in" | "not_in", x, values)    values is a tuple of VALUES (numbers, str / bytes, "lit" nodes), not of operands
    ("is_null" | "is_not_null", column)
    ("between" | "not_between", x, low, high)
    ("like" | "not_like", column, ("lit", pattern))
    ("lookup" | "lookup_i32", code column, table column)     what core.lowering makes of LIKE / of two string columns compared
    ("upper" | "lower", string column or another such node)  core.lowering turns it into a derived dictionary-coded column
    ("concat", x, ...)              x: string columns, such nodes, upper / lower nodes, ("lit", s) and numbers; core.lowering turns
                                    it into a derived dictionary-coded column (never NULL: a NULL operand is "None")
    ("to_str", column)              an integer, date32, timestamp or string column, or another string-function node; core.lowering
                                    turns it into a derived dictionary-coded column (never NULL: a NULL row is "None")
    ("date", x)                     x: a string column or string-function node (parsed once per distinct value), a date32 / timestamp
    ("datetime", x[, ("lit", unit)])  column (a change of unit), for from_timestamp an integer column (its values as timestamps), or a
    ("from_timestamp", x[, ("lit", unit)])  literal.  core.lowering turns the node into a derived date32 / timestamp[unit] column WITH
                                    validity ('' and NaT are NULL); units: date D; datetime D s ms us ns (default s over a column);
                                    from_timestamp s ms us ns (default s).  The unit is no operand.  Over a literal the node folds
                                    into a ("temporal", ...) constant (fold_temporal)
    ("temporal", value, unit)       a date / timestamp constant: `value` days (unit D) or unit counts since 1970-01-01.  A leaf.  It
                                    may only stand in a comparison (or BETWEEN) with a temporal operand: core.lowering aligns units
    ("timedelta", n[, ("lit", unit)])  n an integer literal; folds into a ("duration", ...) constant (fold_timedelta)
    ("duration", value, unit)       a timedelta constant: `value` counts of `unit` -- D s ms us ns, or None (NumPy's generic
                                    timedelta, which takes the unit of the operand it meets).  A leaf
    ("now",)                        the instant of planning: fold_now replaces it ONCE per query with ("temporal", seconds, "s")
    ("is_busday", x[, ("lit", weekmask)[, (date string, ...)]])  x: a date32 column or a date() node; core.lowering turns it into
                                    a predicate over a mask column (np.is_busday; a NULL row is False)
    ("floordiv" | "//", x, y)       duration // duration -> an int64 column with validity (vnm_temporal_floordiv); no other operands
    add / sub / mul / div / neg     over temporal and duration operands follow NumPy's datetime64 / timedelta64 rules
                                    (core.lowering): the node becomes a derived column or a constant
    ("fn", name, arg...)            a function by name (planner: the aggregates); name is no operand

"lit", "strong", "temporal", "duration" and "now" nodes are leaves.  Pass-through nodes keep the spelling they came with (`(">", "v", "w")` stays that):
an operator is canonicalised with cmp_name() only where it is matched.  A new operator is added to ops._EX (and to
core.lowering._ARITHMETIC when it takes numbers); a new node FORM is a line above and, unless its operands are e[1:], in _OPERANDS.
No ctypes, no library, no device: this module imports without them.
"""
import numpy as np

# comparison spellings -> canonical name; every other comparison table of the package is derived from this one or stands below
CMP_SYMBOLS = {"==": "eq", "=": "eq", "!=": "ne", "<>": "ne", ">": "gt", ">=": "ge", "<": "lt", "<=": "le"}
CMP_SYMBOL = {n: s for s, n in reversed(CMP_SYMBOLS.items())}              # name -> its first symbol: "eq" -> "=="
CMP_FLIP = {"eq": "eq", "ne": "ne", "lt": "gt", "le": "ge", "gt": "lt", "ge": "le"}          # a < b  <=>  b > a
IN_OPS = ("in", "not_in")
# where the operands stand, by a node's first slot (the walkers slice with it themselves: operands() is a call more per node)
_REST, _NONE = slice(1, None), slice(0, 0)
_OPERANDS = {"lit": _NONE, "strong": _NONE, "temporal": _NONE, "duration": _NONE, "now": _NONE, "in": slice(1, 2), "not_in": slice(1, 2),
             "fn": slice(2, None), "date": slice(1, 2), "datetime": slice(1, 2), "from_timestamp": slice(1, 2), "timedelta": slice(1, 2),
             "is_busday": slice(1, 2)}


def cmp_name(op):
    """The canonical name ("eq" ... "ge") of a comparison operator in either spelling, None for any other operator."""
    return CMP_SYMBOLS.get(op, op if op in CMP_FLIP else None)


def is_number(e) -> bool:
    return (isinstance(e, (int, float)) and not isinstance(e, bool)) or (isinstance(e, tuple) and len(e) == 2 and e[0] == "strong")


def is_str_lit(e) -> bool:
    return isinstance(e, tuple) and len(e) == 2 and e[0] == "lit" and isinstance(e[1], (str, bytes))


def operands(e) -> tuple:
    """The sub-expressions of a node (none for a column, a number and the "lit" / "strong" leaves)."""
    return e[_OPERANDS.get(e[0], _REST)] if isinstance(e, tuple) and e else ()


def with_operands(e, new):
    """`e` over as many operands `new`; `e` ITSELF when every one `is` the old one (passes identify nodes by id())."""
    where = _OPERANDS.get(e[0], _REST) if isinstance(e, tuple) and e else _NONE
    if len(new) != len(e[where]):
        raise ValueError(f"{e!r} has {len(e[where])} operand(s), not {len(new)}")
    return e if all(a is b for a, b in zip(e[where], new)) else e[:where.start] + tuple(new) + (e[where.stop:] if where.stop else ())


def transform(e, f):
    """Rebuild `e` bottom-up: f(node) may replace a node (tuples only, the leaves included; operands first)."""
    if not isinstance(e, tuple):
        return e
    where, new = _OPERANDS.get(e[0], _REST), None
    for i, x in enumerate(e[where]):
        if isinstance(x, tuple) and (y := transform(x, f)) is not x:
            new = list(e[where]) if new is None else new        # no list while nothing changes: the usual case
            new[i] = y
    return f(e if new is None else with_operands(e, new))


def rewrite(e, f):
    """Rebuild `e` top-down: what f(node) returns is finished, on None the walk goes on into the operands; f sees operator nodes only."""
    where = _OPERANDS.get(e[0], _REST) if isinstance(e, tuple) and e else _NONE
    r, new = (f(e) if where is not _NONE else e), None
    if r is not None:
        return r
    for i, x in enumerate(e[where]):
        if isinstance(x, tuple) and (y := rewrite(x, f)) is not x:
            new = list(e[where]) if new is None else new
            new[i] = y
    return e if new is None else with_operands(e, new)


def nodes(e) -> list:
    """Every sub-expression of `e`, itself first (pre-order): columns, numbers and leaves included."""
    out = [e]
    for x in (e[_OPERANDS.get(e[0], _REST)] if isinstance(e, tuple) and e else ()):
        if isinstance(x, tuple):
            out += nodes(x)
        else:
            out.append(x)
    return out


def columns_of(expr):
    """Column names referenced by a (possibly sugared) expression, in first-use order."""
    return list(dict.fromkeys([n for n in nodes(expr) if isinstance(n, str)]))


def desugar(e):
    """BETWEEN / IN rewrite onto the primitive predicates, exactly what the reference's callables compute:
    between -> logical_and(x >= low, x <= high), not_between -> logical_or(x < low, x > high)
    (vinum/core/expressions.py:43-48); in / not_in -> np.isin(x, values[, invert]) (:39-40)."""
    def f(n):
        if n[0] == "between":
            return ("and", ("ge", n[1], n[2]), ("le", n[1], n[3]))
        if n[0] == "not_between":
            return ("or", ("lt", n[1], n[2]), ("gt", n[1], n[3]))
        if n[0] not in IN_OPS:
            return n
        vals = list(n[2])
        if not vals:
            raise ValueError("IN with an empty list")
        # np.isin turns the list into an ARRAY (int64 / float64: strong types), unlike a bare literal operand
        if any(isinstance(v, float) for v in vals):
            vals = [float(v) for v in vals]
        chain, cmp = ("or", "eq") if n[0] == "in" else ("and", "ne")
        terms = tuple((cmp, n[1], ("strong", v)) for v in vals)
        return (chain,) + terms if len(terms) > 1 else terms[0]
    return transform(e, f)


# The numeric built-ins of the reference's _default_functions_registry (vinum/core/functions.py:353-387) with the callables
# it registers: what a subtree of literals folds to on the host, so folded constants keep NumPy's value AND scalar type
# (np.sqrt(4) is a strong np.float64, pi() the weak Python float np.pi)
SCALAR_FUNCS = {
    "abs": np.absolute, "sqrt": np.sqrt, "cos": np.cos, "sin": np.sin, "tan": np.tan, "power": np.power,
    "log": np.log, "log2": np.log2, "log10": np.log10,
    "to_int": lambda x: np.array(x, dtype="int"), "to_float": lambda x: np.array(x, dtype="float"),
    "to_bool": lambda x: np.array(x, dtype="bool"),
    "pi": lambda: np.pi, "e": lambda: np.e,
}
SCALAR_ARITY = {"power": 2, "pi": 0, "e": 0}


def _lit_value(e):
    """a literal operand as the Python / NumPy scalar the reference's ufunc receives"""
    if isinstance(e, tuple):
        return np.float64(e[1]) if isinstance(e[1], float) else np.int64(e[1])
    return e


def fold(e):
    """Fold every built-in function whose operands are all literals, with NumPy itself."""
    def f(n):
        if n[0] not in SCALAR_FUNCS or not all(is_number(a) for a in n[1:]):
            return n
        with np.errstate(all="ignore"):
            v = SCALAR_FUNCS[n[0]](*[_lit_value(a) for a in n[1:]])
        if isinstance(v, float) and not isinstance(v, np.floating):
            return v                                   # pi() / e(): a weak Python float
        v = np.asarray(v)
        if v.dtype == np.bool_:
            raise TypeError("boolean literals are not arithmetic operands")
        if v.dtype == np.float64:
            return ("strong", float(v))
        if v.dtype == np.int64:
            return ("strong", int(v))
        raise TypeError(f"a constant of type {v.dtype} is not supported")
    return transform(e, f)


# The datetime built-ins (vinum/core/functions.py:25-137, registered at :376-379): name -> (the reference's class name, its UNITS in
# increasing resolution, its default unit -- None: NumPy picks one from the text)
TEMPORAL_FNS = {"date": ("DateFunction", ("D",), "D"), "datetime": ("DatetimeFunction", ("D", "s", "ms", "us", "ns"), None),
                "from_timestamp": ("TimestampFunction", ("s", "ms", "us", "ns"), "s")}
_NUMPY_UNITS = ("Y", "M", "W", "D", "h", "m", "s", "ms", "us", "ns")


def temporal_unit_arg(e):
    """The unit a date / datetime / from_timestamp node asks for: its ("lit", unit) argument checked against the function's list
    (DatetimeFunction._ensure_ts_unit's message, as ValueError), else the function's default (None: datetime() without one)."""
    cls, units, default = TEMPORAL_FNS[e[0]]
    if len(e) < 2 or len(e) > 3:
        raise NotImplementedError(f"no GPU lowering for {e[0]}() with {len(e) - 1} operand(s)")
    if len(e) == 2:
        return default
    unit = e[2][1] if is_str_lit(e[2]) else e[2]
    if not (is_str_lit(e[2]) and isinstance(unit, str) and unit in units):
        raise ValueError(f"Unsupported {cls} unit: '{unit}'. Supported units are: [{', '.join(units)}]")
    return unit


def fold_temporal(e):
    """A date / datetime / from_timestamp node over a LITERAL -> ("temporal", value, unit), computed by NumPy itself with the
    reference's unit rules (DatetimeFunction._expr_kernel + _ensure_unit_correctness: a unit NumPy picked that the function does not
    list -- Y, M, h, m -- is raised to the next finer one it lists).  None when the operand is no literal."""
    x = e[1] if len(e) > 1 else None
    if not (is_str_lit(x) or (isinstance(x, (int, np.integer)) and not isinstance(x, bool))):
        return None
    _, units, _ = TEMPORAL_FNS[e[0]]
    unit = temporal_unit_arg(e)
    v = x[1] if is_str_lit(x) else int(x)
    if isinstance(v, bytes):
        v = v.decode("utf-8")
    arr = np.array(v, dtype=f"datetime64[{unit}]" if unit else "datetime64")
    name = arr.dtype.name
    got = name[name.index("[") + 1:name.index("]")] if "[" in name else ""
    if got not in units:
        finer = [u for u in _NUMPY_UNITS[_NUMPY_UNITS.index(got) + 1:] if u in units] if got in _NUMPY_UNITS else []
        got = finer[0] if finer else units[-1]
        arr = arr.astype(f"datetime64[{got}]")
    if np.isnat(arr):
        raise NotImplementedError(f"no GPU lowering for the constant {e[0]}({v!r}): it is NaT, which compares False with everything")
    return ("temporal", int(arr.astype(np.int64)), got)


# timedelta(n[, unit]) (np.timedelta64, functions.py:380): the units a constant may carry.  Arrow has no duration unit coarser than the
# second and NumPy cannot add months or years to days, so W becomes 7 D, h and m become s, Y and M are refused
_TIMEDELTA_UNITS = {"W": ("D", 7), "D": ("D", 1), "h": ("s", 3600), "m": ("s", 60), "s": ("s", 1), "ms": ("ms", 1), "us": ("us", 1), "ns": ("ns", 1)}
TEMPORAL_ARITH = {"add": "add", "+": "add", "sub": "sub", "-": "sub", "mul": "mul", "*": "mul", "div": "div", "/": "div", "mod": "mod",
                  "%": "mod", "neg": "neg", "floordiv": "floordiv", "//": "floordiv"}


def fold_timedelta(e):
    """A timedelta node -> ("duration", value, unit): unit D / s / ms / us / ns, or None without one (NumPy's generic timedelta).
    n must be an integer literal: a column operand raises NotImplementedError, a float or string TypeError as np.timedelta64 does."""
    if len(e) < 2 or len(e) > 3:
        raise NotImplementedError(f"no GPU lowering for timedelta() with {len(e) - 1} operand(s)")
    n = e[1][1] if isinstance(e[1], tuple) and len(e[1]) == 2 and e[1][0] == "strong" else e[1]
    if isinstance(n, (str, tuple)) and not is_str_lit(n):
        raise NotImplementedError(f"no GPU lowering for timedelta() over {n!r}: the count must be an integer literal, not a column or an expression")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError(f"timedelta() takes an integer count, not {n!r}")
    if len(e) == 2:
        return ("duration", int(n), None)
    unit = e[2][1] if is_str_lit(e[2]) else e[2]
    if isinstance(unit, bytes):
        unit = unit.decode("utf-8")
    if unit in ("Y", "M"):
        raise ValueError(f"timedelta() with the unit {unit!r}: years and months have no fixed length, NumPy cannot add them to days either")
    if not (isinstance(unit, str) and unit in _TIMEDELTA_UNITS):
        raise ValueError(f"Unsupported timedelta unit: '{unit}'. Supported units are: [{', '.join(_TIMEDELTA_UNITS)}]")
    to, k = _TIMEDELTA_UNITS[unit]
    v = int(n) * k
    if not -2**63 < v < 2**63:
        raise OverflowError(f"timedelta({n}, {unit!r}) does not fit int64 in the unit {to!r}")
    return ("duration", v, to)


def now_seconds() -> int:
    """what now() folds to: np.datetime64('now'), whole seconds since 1970-01-01"""
    import time
    return int(time.time())


def fold_now(exprs):
    """The expressions of ONE query (None entries pass) with every ("now",) node replaced by the same ("temporal", seconds, "s")
    constant: a query sees a single instant (the reference evaluates np.datetime64('now') once per batch).  The clock is read once,
    and only when a now() occurs."""
    is_now = lambda n: isinstance(n, tuple) and len(n) == 1 and n[0] == "now"
    if not any(is_now(n) for e in exprs if e is not None for n in nodes(e)):
        return list(exprs)
    const = ("temporal", now_seconds(), "s")
    return [e if e is None else transform(e, lambda n: const if is_now(n) else n) for e in exprs]


def temporal_scalar(x):
    """a ("temporal", ...) / ("duration", ...) constant as the NumPy scalar it stands for (a generic duration: np.timedelta64(n))"""
    if x[0] == "temporal":
        return np.datetime64(x[1], x[2])
    return np.timedelta64(x[1], x[2]) if x[2] else np.timedelta64(x[1])


def temporal_const(v):
    """the NumPy datetime64 / timedelta64 scalar `v` as a constant node; its unit is one of D s ms us ns (or generic)"""
    name = np.dtype(v.dtype).name
    unit = name[name.index("[") + 1:name.index("]")] if "[" in name else None
    if np.isnat(v):
        raise NotImplementedError("no GPU lowering for a temporal constant expression that is NaT")
    return ("temporal" if v.dtype.kind == "M" else "duration", int(v.astype(np.int64)), unit)
