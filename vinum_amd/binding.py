"""Seam B2: the reference's Python-level filter / projection dispatch, bound to the device kernels.

In the reference, filter and projection never cross into native code: the planner turns every SQL
expression into a tree of `VectorizedExpression` objects (vinum/core/base.py:89-125) whose `_function` comes from the
registry `EXPRESSION_FUNCTIONS: {SQLExpression: (callable, FunctionType)}` (vinum/core/expressions.py:12-52), and
`Operator.next()` evaluates that tree node by node with NumPy / pyarrow.compute before `FilterOperator._kernel` calls
`RecordBatch.filter(mask)` (vinum/core/algebra.py:108-123, vinum/arrow/record_batch.py:85-90).

This module is what a Vinum maintainer adds to run those operators on the GPU WITHOUT touching the planner:

  * `lower(tree, registry)` reads a VectorizedExpression-SHAPED tree -- anything with the attributes the reference's
    classes have (`arguments`, `_function`, `_is_binary_func`; `Column.get_column_name()`; `Literal.value`;
    `AggregateFunction.get_agg_func_name()` / `get_input_column_name()`) -- identifies each node's SQL operator by the
    identity of its callable in the registry, honours the left fold of binary operators (base.py:145-151) and returns the
    prefix form `vnm_project` / `vnm_filter_*` programs are compiled from (vinum_amd.ops.compile_expr).
  * `device_filter(batch, predicate)` is the `RecordBatch.filter` replacement: predicate tree -> ONE fused mask kernel ->
    one compaction pass over every column (or `vnm_filter_cmp` alone for `column <op> literal`), NULL mask entries and
    NaN comparisons as record_batch.py:85-90,112-118.
  * `GpuFilterOperator` / `GpuProjectOperator` take the reference's constructor arguments (a VectorizedExpression
    predicate; a list of Column / Literal / VectorizedExpression arguments + col_names + keep_input_table) and implement
    the reference's `next()` generator protocol over HBM-resident batches.
  * `install(vinum_pkg)` rebinds the operator names the planner instantiates (vinum/planner/planner.py:16-31) to the GPU
    operators of this package; `QueryPlanner.plan_query` itself stays untouched.

`SQLExpression`, `EXPRESSION_FUNCTIONS`, `Column`, `Literal`, `VectorizedExpression`, `AggregateFunction` below are this
package's own mirror of that contract (same member names, the same third-party callables) -- the reference does not
travel to the GPU box, so tests build trees with the mirror and, in the build container, with the reference's own
planner; both must lower to the same programs.
"""
import enum
from functools import partial
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from . import expr as E
from . import ops
from .core.base import DeviceRecordBatch, Operator


# ---- mirror of the expression contract -----------------------------------------------------------------------
class SQLExpression(enum.Enum):   # vinum/parser/query.py:17-59 (the members the hot path uses)
    ADDITION = enum.auto(); SUBTRACTION = enum.auto(); MULTIPLICATION = enum.auto(); DIVISION = enum.auto()
    MODULUS = enum.auto(); NEGATION = enum.auto(); BINARY_NOT = enum.auto(); BINARY_AND = enum.auto()
    BINARY_OR = enum.auto(); BINARY_XOR = enum.auto()
    EQUALS = enum.auto(); NOT_EQUALS = enum.auto(); GREATER_THAN = enum.auto(); GREATER_THAN_OR_EQUAL = enum.auto()
    LESS_THAN = enum.auto(); LESS_THAN_OR_EQUAL = enum.auto()
    AND = enum.auto(); BETWEEN = enum.auto(); NOT_BETWEEN = enum.auto(); IN = enum.auto(); NOT_IN = enum.auto()
    NOT = enum.auto(); OR = enum.auto(); IS_NULL = enum.auto(); IS_NOT_NULL = enum.auto()
    FUNCTION = enum.auto()
    CONCAT = enum.auto()              # `a || b` (parser.py:81)


class FunctionType(enum.Enum):    # vinum/core/functions.py:347-350
    ARROW = enum.auto()
    NUMPY = enum.auto()
    CLASS = enum.auto()


# the same third-party callables the reference registers (vinum/core/expressions.py:12-52): NumPy ufuncs, comparison
# lambdas, pyarrow.compute kernels
EXPRESSION_FUNCTIONS = {
    SQLExpression.NEGATION: (np.negative, FunctionType.NUMPY),
    SQLExpression.BINARY_NOT: (lambda x: ~x, FunctionType.NUMPY),
    SQLExpression.BINARY_AND: (np.bitwise_and, FunctionType.NUMPY),
    SQLExpression.BINARY_OR: (np.bitwise_or, FunctionType.NUMPY),
    SQLExpression.BINARY_XOR: (np.bitwise_xor, FunctionType.NUMPY),
    SQLExpression.ADDITION: (np.add, FunctionType.NUMPY),
    SQLExpression.SUBTRACTION: (np.subtract, FunctionType.NUMPY),
    SQLExpression.MULTIPLICATION: (np.multiply, FunctionType.NUMPY),
    SQLExpression.DIVISION: (np.divide, FunctionType.NUMPY),
    SQLExpression.MODULUS: (np.mod, FunctionType.NUMPY),
    SQLExpression.AND: (pc.and_, FunctionType.ARROW),
    SQLExpression.OR: (pc.or_, FunctionType.ARROW),
    SQLExpression.NOT: (pc.invert, FunctionType.ARROW),
    SQLExpression.EQUALS: (lambda x, y: x == y, FunctionType.NUMPY),
    SQLExpression.NOT_EQUALS: (lambda x, y: x != y, FunctionType.NUMPY),
    SQLExpression.GREATER_THAN: (lambda x, y: x > y, FunctionType.NUMPY),
    SQLExpression.GREATER_THAN_OR_EQUAL: (lambda x, y: x >= y, FunctionType.NUMPY),
    SQLExpression.LESS_THAN: (lambda x, y: x < y, FunctionType.NUMPY),
    SQLExpression.LESS_THAN_OR_EQUAL: (lambda x, y: x <= y, FunctionType.NUMPY),
    SQLExpression.IS_NULL: (pc.is_null, FunctionType.ARROW),
    SQLExpression.IS_NOT_NULL: (pc.is_valid, FunctionType.ARROW),
    SQLExpression.IN: (np.isin, FunctionType.NUMPY),
    SQLExpression.NOT_IN: (partial(np.isin, invert=True), FunctionType.NUMPY),
    SQLExpression.BETWEEN: (lambda x, low, high: np.logical_and(x >= low, x <= high), FunctionType.NUMPY),
    SQLExpression.NOT_BETWEEN: (lambda x, low, high: np.logical_or(x < low, x > high), FunctionType.NUMPY),
}
BINARY_EXPRESSIONS = {SQLExpression.ADDITION, SQLExpression.SUBTRACTION, SQLExpression.MULTIPLICATION, SQLExpression.DIVISION,
                      SQLExpression.MODULUS, SQLExpression.AND, SQLExpression.OR, SQLExpression.EQUALS, SQLExpression.NOT_EQUALS,
                      SQLExpression.GREATER_THAN, SQLExpression.GREATER_THAN_OR_EQUAL, SQLExpression.LESS_THAN,
                      SQLExpression.LESS_THAN_OR_EQUAL}       # vinum/core/expressions.py:55-69


class Column:
    def __init__(self, name: str):
        self._name = name

    def get_column_name(self) -> str:
        return self._name


class Literal:
    def __init__(self, value: Any):
        self._value = value

    @property
    def value(self):
        return self._value


class VectorizedExpression:
    """Shape of vinum/core/base.py:89-125: arguments + the registry callable + the two dispatch flags."""

    def __init__(self, arguments: Iterable, function=None, is_numpy_func: bool = False, is_binary_func: bool = False):
        self._arguments = tuple(arguments)
        self._function = function
        self._is_numpy_function = is_numpy_func
        self._is_binary_func = is_binary_func

    @property
    def arguments(self):
        return self._arguments


class AggregateFunction(VectorizedExpression):
    """Shape of vinum/core/aggregate.py:12-29."""

    def __init__(self, func: str, column: Optional[Column] = None):
        super().__init__([])
        self._func = func
        self._input_column_name = column.get_column_name() if column else ""

    def get_input_column_name(self) -> str:
        return self._input_column_name

    def get_agg_func_name(self) -> str:
        return self._func.upper()


# ---- mirror of the numeric built-in functions (vinum/core/functions.py:148-186, 353-387) ---------------------------
class AbstractCastFunction(VectorizedExpression):
    """Shape of functions.py:148-162: a VectorizedExpression subclass built as Cls(arguments) -- `_function` is None, the
    cast lives in `_expr_kernel` as np.array(x, dtype=type)."""
    type: Optional[str] = None

    def __init__(self, arguments: Iterable, shared_id: Optional[str] = None):
        super().__init__(arguments)


class BoolCastFunction(AbstractCastFunction):
    type = "bool"


class FloatCastFunction(AbstractCastFunction):
    type = "float"


class IntCastFunction(AbstractCastFunction):
    type = "int"


class StringCastFunction(AbstractCastFunction):
    """functions.py:189-193: np.array(x, dtype='str'), NumPy's text of the value."""
    type = "str"


_CAST_SPEC = {"bool": "to_bool", "float": "to_float", "int": "to_int", "str": "to_str"}
_CAST_CLASSES = ("BoolCastFunction", "FloatCastFunction", "IntCastFunction", "StringCastFunction")


class LikeFunction(VectorizedExpression):
    """Shape of functions.py:301-344: LikeFunction((column, Literal(pattern)), invert) -- `_function` is None, the regex match
    lives in `_expr_kernel`; invert = True is NOT LIKE (planner.py:189-193)."""

    def __init__(self, arguments, invert: bool) -> None:
        super().__init__(arguments, is_numpy_func=True)
        self.invert = invert



class AbstractStringFunction(VectorizedExpression):
    """Shape of functions.py:196-247: built as Cls(arguments), `_function` is None, the work lives in `_expr_kernel`."""

    def __init__(self, arguments: Iterable, shared_id: Optional[str] = None):
        super().__init__(arguments)


class UpperStringFunction(AbstractStringFunction):
    """functions.py:279-287: pc.utf8_upper over the argument (cast to string first, :219-221)."""


class LowerStringFunction(AbstractStringFunction):
    """functions.py:290-297: pc.utf8_lower."""


class ConcatFunction(AbstractStringFunction):
    """functions.py:250-276: every argument through np.array(., dtype='U'), folded left with np.char.add -- built as
    Cls(arguments) with the callable and both dispatch flags set."""

    def __init__(self, arguments: Iterable) -> None:
        VectorizedExpression.__init__(self, arguments, function=np.char.add, is_numpy_func=True, is_binary_func=True)


class DatetimeFunction(VectorizedExpression):
    """Shape of functions.py:25-119: built as Cls(arguments) -- (x) or (x, Literal(unit)) --, `_function` is None, the work
    (np.array(x, dtype='datetime64[unit]')) lives in `_expr_kernel`."""

    def __init__(self, arguments: Iterable, shared_id: Optional[str] = None):
        super().__init__(arguments)


class DateFunction(DatetimeFunction):
    """functions.py:122-128: unit D only."""


class TimestampFunction(DatetimeFunction):
    """functions.py:131-137: from_timestamp, units s / ms / us / ns, default s."""


class NowFunction(DatetimeFunction):
    """functions.py:140-145: np.array(['now'], dtype='datetime64'), evaluated per batch there -- here folded once per query."""


_CASE_SPEC = {"UpperStringFunction": "upper", "LowerStringFunction": "lower"}
_TEMPORAL_SPEC = {"DateFunction": "date", "DatetimeFunction": "datetime", "TimestampFunction": "from_timestamp"}
_STRING_FN_NAMES = ("upper", "lower", "concat")       # their "fn" spelling builds what it always built; the operator node builds the class
EXPRESSION_FUNCTIONS[SQLExpression.CONCAT] = (ConcatFunction, FunctionType.CLASS)       # expressions.py:51

# the numeric part of _default_functions_registry, with the same callables (math constants: the lambdas themselves), the three
# string functions and the four casts that run on the device
FUNCTIONS_REGISTRY = {
    "upper": (UpperStringFunction, FunctionType.CLASS),
    "lower": (LowerStringFunction, FunctionType.CLASS),
    "concat": (ConcatFunction, FunctionType.CLASS),
    "to_bool": (BoolCastFunction, FunctionType.CLASS),
    "to_float": (FloatCastFunction, FunctionType.CLASS),
    "to_int": (IntCastFunction, FunctionType.CLASS),
    "to_str": (StringCastFunction, FunctionType.CLASS),
    "date": (DateFunction, FunctionType.CLASS),
    "datetime": (DatetimeFunction, FunctionType.CLASS),
    "from_timestamp": (TimestampFunction, FunctionType.CLASS),
    "now": (NowFunction, FunctionType.CLASS),
    "timedelta": (np.timedelta64, FunctionType.NUMPY),
    "is_busday": (np.is_busday, FunctionType.NUMPY),
    "abs": (np.absolute, FunctionType.NUMPY),
    "sqrt": (np.sqrt, FunctionType.NUMPY),
    "cos": (np.cos, FunctionType.NUMPY),
    "sin": (np.sin, FunctionType.NUMPY),
    "tan": (np.tan, FunctionType.NUMPY),
    "power": (np.power, FunctionType.NUMPY),
    "log": (np.log, FunctionType.NUMPY),
    "log2": (np.log2, FunctionType.NUMPY),
    "log10": (np.log10, FunctionType.NUMPY),
    "pi": (lambda: np.pi, FunctionType.NUMPY),
    "e": (lambda: np.e, FunctionType.NUMPY),
}
_NUMERIC_FNS = tuple(FUNCTIONS_REGISTRY)
# ufuncs are recognised by identity, whatever spelling reached them (`np.sin`, `np.abs` is np.absolute)
_UFUNC_SPEC = {id(fn): name for name, (fn, ft) in FUNCTIONS_REGISTRY.items() if isinstance(fn, np.ufunc)}
# timedelta and is_busday are NumPy's own callables (functions.py:380-381), recognised by identity like the ufuncs
_UFUNC_SPEC.update({id(np.timedelta64): "timedelta", id(np.is_busday): "is_busday"})

_SPEC_TO_SQL = {"add": "ADDITION", "sub": "SUBTRACTION", "mul": "MULTIPLICATION", "div": "DIVISION", "mod": "MODULUS",
                "neg": "NEGATION", "bnot": "BINARY_NOT", "band": "BINARY_AND", "bor": "BINARY_OR", "bxor": "BINARY_XOR",
                "eq": "EQUALS", "ne": "NOT_EQUALS", "gt": "GREATER_THAN", "ge": "GREATER_THAN_OR_EQUAL", "lt": "LESS_THAN",
                "le": "LESS_THAN_OR_EQUAL", "and": "AND", "or": "OR", "not": "NOT", "is_null": "IS_NULL",
                "is_not_null": "IS_NOT_NULL", "in": "IN", "not_in": "NOT_IN", "between": "BETWEEN",
                "not_between": "NOT_BETWEEN", "concat": "CONCAT"}
_SQL_TO_SPEC = {v: k for k, v in _SPEC_TO_SQL.items()}


_AGG_NAMES = ("count_star", "count", "sum", "avg", "min", "max", "np.min", "np.max", "np.sum")


def _is_builtin(name, functions=None):
    """a numeric built-in (or an existing np.<ufunc>) -- any other ("fn", name) stays an AggregateFunction node, as before"""
    if name.startswith("np."):
        return isinstance(getattr(np, name[3:], None), np.ufunc)
    return name in (functions or FUNCTIONS_REGISTRY)


def vectorize(expr, registry=None, classes=None, functions=None, like_cls=None):
    """Build the VectorizedExpression tree the planner builds for `expr` (QueryPlanner._process_expressions_tree,
    vinum/planner/planner.py:140-222) from the prefix form -- with this module's mirror classes by default, or with the
    reference's own (classes = (Column, Literal, VectorizedExpression, AggregateFunction, SQLExpression, FunctionType,
    BINARY_EXPRESSIONS), registry = its EXPRESSION_FUNCTIONS, like_cls = its LikeFunction) in the build container."""
    registry = registry or EXPRESSION_FUNCTIONS
    like_cls = like_cls or LikeFunction
    C, Lt, VE, AF, SQL, FT, BIN = classes or (Column, Literal, VectorizedExpression, AggregateFunction, SQLExpression,
                                             FunctionType, BINARY_EXPRESSIONS)

    def build(e):
        if isinstance(e, str):
            return C(e)
        if isinstance(e, (int, float)):
            return Lt(e)
        op, args = e[0], e[1:]
        if op == "lit":
            return Lt(args[0])
        if op in ("like", "not_like"):                           # planner.py:189-193
            return like_cls(tuple(build(a) for a in args), op == "not_like")
        if op == "||":                                           # parser.py:81: SQLExpression.CONCAT, a CLASS entry of the expression registry
            cls, _ = registry[SQL[_SPEC_TO_SQL["concat"]]]
            return cls([build(a) for a in args])                 # planner.py:129-131: Cls(arguments)
        # (the "fn" spelling of upper / lower builds what it always built, an AggregateFunction node -- the planner resolves that
        #  spelling by the operand's type, planner._case_by_type; the operator node ("upper", x) builds the function's class)
        if op == "fn" and (args[0].lower() in _AGG_NAMES or args[0].lower() in _STRING_FN_NAMES or not _is_builtin(args[0].lower(), functions)):
            arg = build(args[1]) if len(args) > 1 else None
            return AF(args[0], arg) if arg is not None else AF(args[0])
        if op == "fn" or op in FUNCTIONS_REGISTRY:
            name = args[0].lower() if op == "fn" else op
            fargs = args[1:] if op == "fn" else args
            if name.startswith("np."):
                fn, ftype = getattr(np, name[3:]), FT.NUMPY                 # lookup_udf: eval("np.<name>")
            else:
                fn, ftype = (functions or FUNCTIONS_REGISTRY)[name]
            if name == "is_busday" and len(fargs) > 2:                      # the holidays: ONE Literal holding the list, like IN's
                built = [build(a) for a in fargs[:2]] + [Lt([h[1] if isinstance(h, tuple) else h for h in fargs[2]])]
            else:
                built = [build(a) for a in fargs]
            if ftype == FT.CLASS:
                return fn(built)                                            # planner.py:129-131: Cls(arguments)
            return VE(built, function=fn, is_numpy_func=(ftype == FT.NUMPY), is_binary_func=False)
        member = SQL[_SPEC_TO_SQL[op]]
        fn, ftype = registry[member]
        if op in ("in", "not_in"):
            built = [build(args[0]), Lt(list(args[1]))]          # parser.py:151-160: ONE Literal holding the list
        else:
            built = [build(a) for a in args]
        return VE(built, function=fn, is_numpy_func=(ftype == FT.NUMPY), is_binary_func=(member in BIN))
    return build(expr)


# ---- the adapter ---------------------------------------------------------------------------------------------------
def registry_index(expression_functions, functions_registry=None) -> Dict[int, str]:
    """id(callable) -> SQL operator name, for any registry with the reference's layout; with a functions registry
    (_default_functions_registry's layout, name -> (callable, FunctionType)) its numeric built-ins join as "fn:<name>"."""
    index = {id(fn): member.name for member, (fn, _ftype) in expression_functions.items()}
    for name, (fn, _ftype) in (functions_registry or {}).items():
        if name in _NUMERIC_FNS and not isinstance(fn, type):
            index[id(fn)] = "fn:" + name
    return index


_DEFAULT_INDEX = registry_index(EXPRESSION_FUNCTIONS, FUNCTIONS_REGISTRY)


def lower(node, index: Optional[Dict[int, str]] = None):
    """VectorizedExpression-shaped tree -> prefix expression (str | number | tuple) for vinum_amd.ops.  now() folds here, ONCE for
    the whole tree (expr.fold_now): every occurrence is the same instant, and so is every batch."""
    return lower_all([node], index)[0]


def lower_all(nodes, index: Optional[Dict[int, str]] = None) -> list:
    """lower() of several trees of one operator (a SELECT list) under ONE now()"""
    return E.fold_now([_lower_tree(n, index) for n in nodes])


def _lower_tree(node, index: Optional[Dict[int, str]] = None):
    index = index or _DEFAULT_INDEX
    if node is None:
        return None
    if isinstance(node, (bool, int, float, str)):
        return node
    if hasattr(node, "get_agg_func_name"):                     # AggregateFunction (vinum/core/aggregate.py:12-29)
        name = node.get_agg_func_name().lower()
        col = node.get_input_column_name()
        return ("fn", name, col) if col else ("fn", name)
    if hasattr(node, "arguments") and hasattr(node, "_function"):
        fn = node._function
        if fn is None and type(node).__name__ == "LikeFunction":
            like = _lower_like(node, index)
            if like is not None:
                return like
        cast = getattr(type(node), "type", None)
        if fn is None and cast in _CAST_SPEC and type(node).__name__ in _CAST_CLASSES:
            args = [_lower_tree(a, index) for a in node.arguments]   # AbstractCastFunction (functions.py:148-162)
            return (_CAST_SPEC[cast],) + tuple(args)
        # UpperStringFunction / LowerStringFunction (functions.py:279-298), by QUALIFIED name: the class the reference (or this
        # module) defines under that name at module level -- some other class whose __name__ was set to it is not that function
        if fn is None and type(node).__qualname__ in _CASE_SPEC and len(tuple(node.arguments)) == 1:
            return (_CASE_SPEC[type(node).__qualname__], _lower_tree(tuple(node.arguments)[0], index))
        # NowFunction (functions.py:140-145), by qualified name: the ("now",) leaf lower() folds
        if fn is None and type(node).__qualname__ == "NowFunction" and len(tuple(node.arguments)) == 0:
            return ("now",)
        # DateFunction / DatetimeFunction / TimestampFunction (functions.py:25-137), by qualified name as above: (x) or (x, Literal(unit))
        if fn is None and type(node).__qualname__ in _TEMPORAL_SPEC and 1 <= len(tuple(node.arguments)) <= 2:
            return (_TEMPORAL_SPEC[type(node).__qualname__],) + tuple(_lower_tree(a, index) for a in node.arguments)
        # ConcatFunction (functions.py:250-276; `concat(...)` and `a || b` both build it), by qualified name AND by its shape: it
        # carries a callable (np.char.add) and folds as a binary function.  A VectorizedExpression that merely holds np.char.add is
        # not that function.
        if type(node).__qualname__ == "ConcatFunction" and fn is not None and getattr(node, "_is_binary_func", False) and len(tuple(node.arguments)) >= 1:
            return ("concat",) + tuple(_lower_tree(a, index) for a in node.arguments)
        if fn is not None and id(fn) not in index and id(fn) in _UFUNC_SPEC:
            return (_UFUNC_SPEC[id(fn)],) + tuple(_lower_tree(a, index) for a in node.arguments)
        if fn is None or id(fn) not in index:
            raise NotImplementedError(f"no GPU lowering for {fn if fn is not None else type(node).__name__!r}: the numeric "
                                      "operators and the built-ins abs, sqrt, sin, cos, tan, log, log2, log10, power, pi, e, "
                                      "to_int, to_float, to_bool, to_str, upper / lower / concat of string columns, date / datetime / "
                                      "from_timestamp and LIKE / NOT LIKE against a string literal run on the GPU; UDFs, now, "
                                      "timedelta, is_busday and other np.* functions do not")
        sql = index[id(fn)]
        args = [_lower_tree(a, index) for a in node.arguments]
        if sql.startswith("fn:"):
            return (sql[3:],) + tuple(args)
        op = _SQL_TO_SPEC[sql]
        if op in ("in", "not_in"):
            vals = args[1]
            return (op, args[0], tuple(vals) if isinstance(vals, (list, tuple, np.ndarray)) else (vals,))
        if getattr(node, "_is_binary_func", False) and len(args) > 2:
            return (op,) + tuple(args)                         # left fold (base.py:145-151) == the emitter's n-ary chain
        return (op,) + tuple(args)
    if hasattr(node, "value"):                                 # Literal (vinum/parser/query.py:126-176)
        v = node.value
        if isinstance(v, (str, bytes)):                        # a string literal is not a column name: `city = 'Berlin'`
            return ("lit", v)
        return list(v) if isinstance(v, (list, tuple)) else v
    if hasattr(node, "get_column_name"):                       # Column (:179-233)
        return node.get_column_name()
    raise TypeError(f"Unsupported OperatorArgument type: {type(node)}")     # base.py:52-54


def _lower_like(node, index):
    """LikeFunction((operand, Literal(str)), invert: bool) -> ("like" | "not_like", operand, ("lit", pattern)); any other shape
    of a node with that class name -> None (the caller raises "no GPU lowering")."""
    args = tuple(node.arguments)
    invert = getattr(node, "invert", None)
    if len(args) != 2 or not isinstance(invert, bool):
        return None
    lit = args[1]
    if type(lit).__name__ != "Literal" or not hasattr(lit, "value") or not isinstance(lit.value, str):
        return None
    return ("not_like" if invert else "like", _lower_tree(args[0], index), ("lit", lit.value))


def device_filter(batch: DeviceRecordBatch, predicate) -> DeviceRecordBatch:
    """`RecordBatch.filter(mask)` (vinum/arrow/record_batch.py:85-90) with the mask still an expression: the predicate
    tree becomes ONE fused byte-mask kernel and every column is compacted in one more pass; `column <op> literal` is a
    single fused compare + compact kernel.  NULL operands compare as NaN (record_batch.py:112-118)."""
    from .core.algebra import FilterOperator
    from .planner import _simple_predicate, _t
    expr = _t(predicate) if isinstance(predicate, (tuple, list)) else lower(predicate)
    simple = _simple_predicate(expr)
    return FilterOperator(simple if simple is not None else expr, None)._kernel(batch)


class GpuFilterOperator(Operator):
    """FilterOperator(predicate: VectorizedExpression, parent_operator) -- vinum/core/algebra.py:108-123."""

    def __init__(self, predicate, parent_operator, index: Optional[Dict[int, str]] = None):
        super().__init__(parent_operator)
        self.predicate = lower(predicate, index)

    def _kernel(self, batch: DeviceRecordBatch) -> DeviceRecordBatch:
        return device_filter(batch, self.predicate)


class GpuProjectOperator(Operator):
    """ProjectOperator(arguments, parent_operator, col_names=None, keep_input_table=False) -- algebra.py:28-105.
    Arguments are Column / Literal / VectorizedExpression objects; every computed expression of the list goes into one
    fused kernel (vnm_project_multi)."""

    def __init__(self, arguments, parent_operator, col_names: Optional[Sequence[str]] = None, keep_input_table: bool = False,
                 index: Optional[Dict[int, str]] = None):
        super().__init__(parent_operator)
        from .core.algebra import ProjectOperator
        args = list(arguments)
        exprs = lower_all(args, index)
        if col_names is None:                                   # algebra.py:66-75: the arguments name their columns
            col_names = [a.get_column_name() if hasattr(a, "get_column_name") else f"expr_{i}" for i, a in enumerate(args)]
        self._inner = ProjectOperator(exprs, None, col_names=list(col_names), keep_input_table=keep_input_table)
        self.expressions = exprs

    def _kernel(self, batch: DeviceRecordBatch) -> DeviceRecordBatch:
        return self._inner._kernel(batch)


def install(vinum_pkg) -> None:
    """Rebind the operator classes the reference's planner instantiates (vinum/planner/planner.py:16-31 imports them
    into its namespace) to GPU operators.  After this, QueryPlanner.plan_query builds a plan of GPU operators for
    numeric hot-path queries; nothing in the planner, binder or executor is edited.  (sys.modules['vinum_lib'] =
    vinum_amd.vinum_lib covers the native seam B1, see INTEGRATION.md.)"""
    planner_mod = __import__(vinum_pkg.__name__ + ".planner.planner", fromlist=["x"])
    expr_mod = __import__(vinum_pkg.__name__ + ".core.expressions", fromlist=["x"])
    fn_mod = __import__(vinum_pkg.__name__ + ".core.functions", fromlist=["x"])
    index = registry_index(expr_mod.EXPRESSION_FUNCTIONS, fn_mod._default_functions_registry)

    class _Filter(GpuFilterOperator):
        def __init__(self, predicate, parent_operator):
            super().__init__(predicate, parent_operator, index=index)

    class _Project(GpuProjectOperator):
        def __init__(self, arguments, parent_operator, col_names=None, keep_input_table=False):
            super().__init__(arguments, parent_operator, col_names=col_names, keep_input_table=keep_input_table, index=index)

    planner_mod.FilterOperator = _Filter
    planner_mod.ProjectOperator = _Project
    planner_mod._vinum_amd_index = index
