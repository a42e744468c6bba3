"""What a dictionary-coded column (strings, binaries: int32 codes of the column's own running dictionary in HBM) needs before an
expression over it is a numeric program: four rewrites of vinum_amd.expr trees (lower_dictionary runs them in order) and the one
path on which the operators evaluate lowered expressions (project_lowered, used_columns).  `columns` is a batch's name ->
DeviceColumn; every rewrite returns (expression, extra), `extra` holding the tables, rank and mask columns the result reads by name."""
import hashlib

import numpy as np
import pyarrow as pa

from .. import expr as E
from .. import ops
from .. import keydict as K
from ..keydict import ValueTable, to_str_kind


def _is_dict(x, columns) -> bool:
    return isinstance(x, str) and x in columns and columns[x].dictionary is not None


def value_type_of(dictionary):
    """what a dictionary's VALUES are: a dictionary-typed column (dictionary<int8, utf8>) is a utf8 column to every message and rule"""
    return getattr(dictionary, "value_type", dictionary.type)


def pa_is_string(t) -> bool:
    import pyarrow as pa
    return pa.types.is_string(t) or pa.types.is_large_string(t)


CASE_FNS = ("upper", "lower")
STRING_FNS = CASE_FNS + ("concat", "to_str")
TEMPORAL_FNS = tuple(E.TEMPORAL_FNS)                # date, datetime, from_timestamp
_DERIVED_TEMPORAL = "__temporal_"                   # the name prefix of the date32 / timestamp columns they derive


def with_derived(columns, extra):
    """`columns` plus the columns a lowering has put into `extra` that stand for a node (lower_case_functions: upper(city) is a
    dictionary-coded column, date(d) a date32 column)"""
    derived = {n: c for n, c in extra.items() if getattr(c, "dictionary", None) is not None or n.startswith(_DERIVED_TEMPORAL)}
    return {**columns, **derived} if derived else columns


def concat_literal(x):
    """the bytes a literal operand of concat() contributes (ConcatFunction, functions.py:250-276: np.array(str(x), dtype='U')): a
    string literal without its trailing NULs, a number as str(number); None for anything that is no literal"""
    if E.is_str_lit(x):
        v = x[1]
        return (v.encode("utf-8") if isinstance(v, str) else bytes(v)).rstrip(b"\x00")
    if isinstance(x, (bool, int, float)):
        return str(x).encode("utf-8")
    return None


def lower_case_functions(expr, columns, extra=None):
    """The one pass over the string-function nodes, in any nesting: upper(x) / lower(x) (UpperStringFunction / LowerStringFunction,
    vinum/core/functions.py:279-298: pc.utf8_upper / utf8_lower) and concat(x, ...) (ConcatFunction, :250-276) over dictionary-coded
    string columns, literals and other such nodes.  A node becomes the NAME of a derived column added to `extra` -- the int32 codes
    of a DERIVED dictionary, `.dictionary` that dictionary -- and is to every later step and operator an ordinary string column.  A
    node that occurs several times under one `extra` is materialised once.
      * upper / lower: KeyDictionary.mapped_column -- each distinct value mapped once on the device, a row one lookup, the
        operand's validity.
      * concat: adjacent literals merge here (a number is str(number), a string literal loses its trailing NULs).  One column with
        literals is a function of the value (KeyDictionary.affixed_column: prefix + value + suffix once per distinct value, a row
        one lookup).  Two columns are a function of the row's PAIR of codes (KeyDictionary.pair_column: a persistent device pair
        table, the bytes written once per distinct pair); three or more fold left as the reference does, the first step's derived
        dictionary being the second step's left one, the literal in front of the first column and the one behind the last going
        into the first / last step's byte writer.  The result has no validity: a NULL operand is "None".
      * to_str(x) (StringCastFunction, functions.py:189-193: np.array(x, dtype='str')): over an integer, date32 or timestamp
        column a function of the row's VALUE (keydict.ValueTable.column: a persistent device value table hanging in the scan's
        per-name registry, each distinct value formatted once, a row one probe; a NULL row is "None", no validity); over a string
        column or another such node the value without trailing NULs, which is the empty affix (affixed_column(b"", b"", col)).
    A BARE numeric or temporal column under upper / lower / concat raises TypeError naming it (write to_str(v)), a
    concat() of literals alone and any other operand expression NotImplementedError; a binary column TypeError and a host-route
    dictionary NotImplementedError (KeyDictionary.mapped / affixed / paired).  to_str() of a float, decimal, date64, time, duration,
    boolean or binary column raises TypeError naming the column and its type, of an expression or a literal NotImplementedError.
      * date(x) / datetime(x[, unit]) / from_timestamp(x[, unit]) (DateFunction / DatetimeFunction / TimestampFunction,
        functions.py:25-137: np.array(x, dtype='datetime64[unit]')) become the name of a derived date32 / timestamp[unit] column
        WITH validity and without a dictionary.  Over a string column or a string-function node it is a function of the VALUE
        (KeyDictionary.parsed_column: each distinct value parsed once on the device, a row one lookup; '' and NaT are NULL; a value
        the parser refuses raises ValueError naming it).  Over a date32 / timestamp column it is a change of unit
        (keydict.rescaled_column; the column itself when the unit is its own), over an integer column under from_timestamp the
        same values retyped (keydict.timestamp_column).  datetime(x) without a unit over a column is timestamp[s] -- the reference
        lets NumPy pick the unit batch by batch.  Over a LITERAL the node folds into a ("temporal", value, unit) constant with
        NumPy itself (expr.fold_temporal).  A comparison (BETWEEN too) with such a constant, or of two temporal operands of
        different units, is aligned to the finer unit as NumPy does: the coarser side is multiplied by the factor; durations
        compare with durations the same way.
      * timedelta(n[, unit]) folds into a ("duration", ...) constant (expr.fold_timedelta); add / sub / mul / div / neg over temporal
        and duration operands, is_busday() and IN lists of temporal constants are the stage TemporalArithmetic below.  A temporal
        or duration constant left alone -- in SELECT -- raises NotImplementedError; so does a now() that was not folded at plan time."""
    extra = {} if extra is None else extra

    def operand(fn, x):
        """the name of the string column `x` stands for, its column; None where its dictionary cannot do this (a stub): the node stays"""
        if isinstance(x, tuple) and x and x[0] in STRING_FNS:
            x = f(x)
        cols = with_derived(columns, extra)
        if not isinstance(x, str) or x not in cols:
            raise NotImplementedError(f"no GPU lowering for {fn}() over {x!r}: the operand must be a string column or upper() / lower()" +
                                      (" / concat() of one, or a literal" if fn == "concat" else " of one"))
        c = cols[x]
        if c.dictionary is None:
            raise TypeError(f"{fn}() needs a string column, {x!r} is {c.arrow_type}")
        return x, c

    def case_fn(e):
        if len(e) != 2:
            raise NotImplementedError(f"no GPU lowering for {e[0]}() with {len(e) - 1} operand(s)")
        x, c = operand(e[0], e[1])
        mapped_column = getattr(c.dictionary, "mapped_column", None)
        if mapped_column is None:         # a dictionary object that cannot map: the node stays, and is refused where it is compiled
            return e
        name = f"__{e[0]}_{x}"
        if name not in extra:
            extra[name] = mapped_column(e[0], c)
        return name

    def concat(e):
        parts = []                         # bytes (merged literals) and (name, column) in operand order
        for x in e[1:]:
            lit = concat_literal(x)
            if lit is None:
                parts.append(operand("concat", x))
            elif parts and isinstance(parts[-1], bytes):
                parts[-1] += lit
            else:
                parts.append(lit)
        cols = [p for p in parts if not isinstance(p, bytes)]
        if not cols:
            raise NotImplementedError(f"no GPU lowering for concat() of literals alone ({list(e[1:])!r}): there is no per-row work")
        if any(getattr(c.dictionary, "affixed_column", None) is None or getattr(c.dictionary, "pair_column", None) is None for _, c in cols):
            return e                       # (a dictionary object that cannot concatenate: refused where the node is compiled)
        lits, at = [b""], 0                # lits[k]: the literal in front of column k; lits[len(cols)]: the one behind the last
        for p in parts:
            if isinstance(p, bytes):
                lits[at] = p
            else:
                at += 1
                lits.append(b"")
        label = lambda b: repr(b.decode("utf-8", "replace"))
        (name, col) = cols[0]
        if len(cols) == 1:
            out = f"__concat({label(lits[0])},{name},{label(lits[1])})"
            if out not in extra:
                extra[out] = col.dictionary.affixed_column(lits[0], lits[1], col)
            return out
        for k in range(1, len(cols)):       # the left fold: (((a . b) . c) . d)
            rname, rcol = cols[k]
            prefix, suffix = lits[0] if k == 1 else b"", lits[len(cols)] if k == len(cols) - 1 else b""
            out = f"__concat({label(prefix)},{name},{label(lits[k])},{rname},{label(suffix)})"
            if out not in extra:
                extra[out] = col.dictionary.pair_column(rcol.dictionary, prefix, lits[k], suffix, col, rcol)
            name, col = out, extra[out]
        return name

    def to_str(e):
        if len(e) != 2:
            raise NotImplementedError(f"no GPU lowering for to_str() with {len(e) - 1} operand(s)")
        x = e[1]
        if isinstance(x, tuple) and x and (x[0] in STRING_FNS + TEMPORAL_FNS or x[0] in E.TEMPORAL_ARITH):
            x = lower(x)
        cols = with_derived(columns, extra)
        if not isinstance(x, str) or x not in cols:
            raise NotImplementedError(f"no GPU lowering for to_str() over {x!r}: the operand must be a column or upper() / lower() / concat() / "
                                      "to_str() of one")
        c = cols[x]
        name = f"__to_str_{x}"
        if name in extra:
            return name
        if c.dictionary is None:
            to_str_kind(c.arrow_type, x)                  # (TypeError for a float, decimal, time ... column, naming it)
            extra[name] = ValueTable.of(c, x).column(c)
            return name
        affixed_column = getattr(c.dictionary, "affixed_column", None)
        if affixed_column is None:         # (a dictionary object that cannot concatenate: refused where the node is compiled)
            return e
        if not getattr(c.dictionary, "on_device", True) or not (pa_is_string(value_type_of(c.dictionary))):
            raise TypeError(f"to_str() takes an integer, date32, timestamp or string column, {x!r} is {value_type_of(c.dictionary)}")
        extra[name] = affixed_column(b"", b"", c)
        return name

    def temporal(e):
        fn = e[0]
        unit = E.temporal_unit_arg(e)                     # (ValueError for a unit the function does not list)
        const = E.fold_temporal(e)
        if const is not None:
            return const
        unit = unit or "s"
        x = e[1]
        if isinstance(x, tuple) and x and (x[0] in STRING_FNS + TEMPORAL_FNS or x[0] in E.TEMPORAL_ARITH):
            x = lower(x)
        cols = with_derived(columns, extra)
        if not isinstance(x, str) or x not in cols:
            raise NotImplementedError(f"no GPU lowering for {fn}() over {x!r}: the operand must be a column, upper() / lower() / concat() / to_str() "
                                      "of one, or a literal")
        c = cols[x]
        name = f"{_DERIVED_TEMPORAL}{fn}_{unit}_{x}"
        if name in extra:
            return name
        if c.dictionary is not None:
            parsed_column = getattr(c.dictionary, "parsed_column", None)
            if parsed_column is None:          # (a dictionary object that cannot parse: refused where the node is compiled)
                return e
            extra[name] = parsed_column(unit, c)
            return name
        kind = K.temporal_operand_kind(fn, c.arrow_type, x)        # (TypeError for a float, uint64, decimal ... column, naming it)
        col = K.rescaled_column(c, unit) if kind == "rescale" else K.timestamp_column(c, unit)
        if col is c:
            return x
        extra[name] = col
        return name

    is_const = is_temporal_const
    lower = lambda x: E.rewrite(x, f) if isinstance(x, tuple) else x
    rules = TemporalArithmetic(columns, extra, lower)
    kind_of = rules.kind_of

    def in_unit(x, have, want):
        k = K.UNITS_PER_DAY[want] // K.UNITS_PER_DAY[have]
        if is_const(x):
            v = x[1] * k
            if not -2**63 <= v < 2**63:
                raise OverflowError(f"the temporal constant {x[1]} [{have}] does not fit int64 in the unit {want!r} of the other operand")
            return ("strong", v)
        return x if k == 1 else ("mul", x, ("strong", k))

    def lowered_operands(e):
        return [lower(x) for x in e[1:]]

    def compare(e):
        a, b = lowered_operands(e)
        (ka, ua), (kb, ub) = kind_of(a) or (None, None), kind_of(b) or (None, None)
        if ka and kb and ka != kb:
            raise TypeError(f"cannot compare {rules.describe(a)} with {rules.describe(b)}: a date / timestamp and a duration")
        # a generic duration constant -- timedelta(n) -- takes the unit of the duration it meets
        if kb == "duration" and is_const(a) and ua is None:
            ua = ub
        if ka == "duration" and is_const(b) and ub is None:
            ub = ua
        if not (is_const(a) or is_const(b)) and (ua is None or ub is None or ua == ub):
            return E.with_operands(e, [a, b])
        if is_const(a) and is_const(b):
            raise NotImplementedError(f"no GPU lowering for the comparison of two temporal constants ({a!r}, {b!r}): there is no per-row work")
        for x, u, const in ((a, ua, b), (b, ub, a)):
            if u is None:
                raise TypeError(f"cannot compare the temporal constant {const[1]} [{const[2]}] with {x!r}: only a date32 / timestamp column or "
                                "date() / datetime() / from_timestamp() of a column" + (", or a duration" if const[0] == "duration" else ""))
        want = max(ua, ub, key=K.TEMPORAL_UNITS.index)
        return (e[0], in_unit(a, ua, want), in_unit(b, ub, want))

    def between(e):
        xs = lowered_operands(e)
        units = [(kind_of(x) or (None, None))[1] for x in xs]
        if any(is_const(x) for x in xs) or (all(units) and len(set(units)) > 1):
            x, lo, hi = xs
            return E.rewrite(("and", ("ge", x, lo), ("le", x, hi)) if e[0] == "between" else ("or", ("lt", x, lo), ("gt", x, hi)), f)
        return E.with_operands(e, xs)

    def f(e):
        if e[0] in CASE_FNS:
            return case_fn(e)
        if e[0] == "concat":
            return concat(e)
        if e[0] == "to_str":
            return to_str(e)
        if e[0] in TEMPORAL_FNS:
            return temporal(e)
        if E.cmp_name(e[0]) and len(e) == 3:
            return compare(e)
        if e[0] in ("between", "not_between") and len(e) == 4:
            return between(e)
        if e[0] == "timedelta":
            return E.fold_timedelta(e)
        if e[0] in E.TEMPORAL_ARITH:
            return rules.arithmetic(e)
        if e[0] == "is_busday":
            return rules.is_busday(e)
        if e[0] in E.IN_OPS and len(e) == 3:
            return rules.in_list(e, temporal)
        return None
    out = E.rewrite(expr, f)
    for n in E.nodes(out):
        if is_const(n):
            raise NotImplementedError(f"no GPU lowering for the temporal constant {n[1]} [{n[2]}] outside a comparison or arithmetic with a "
                                      "temporal column: there is no per-row work (alone in SELECT)")
        if isinstance(n, tuple) and n and n[0] == "now":
            raise NotImplementedError("now() reached the per-batch lowering: it folds once per query, at plan time (expr.fold_now)")
    return out, extra


def is_temporal_const(x) -> bool:
    """a ("temporal", value, unit) or ("duration", value, unit) leaf"""
    return isinstance(x, tuple) and len(x) == 3 and x[0] in ("temporal", "duration")


def _is_int(x) -> bool:
    return (isinstance(x, int) and not isinstance(x, bool)) or (isinstance(x, tuple) and len(x) == 2 and x[0] == "strong" and isinstance(x[1], int))


class TemporalArithmetic:
    """The stage of lower_case_functions that types arithmetic over temporal values the way NumPy's datetime64 / timedelta64 do
     and lowers it onto vnm_temporal_affine (keydict.affine_column): out = a * ka + b * kb + c, exact in int64,
    with validity.  The kinds: "temporal" [D s ms us ns] -- a date32 / timestamp column, a derived one, a ("temporal", ...) constant --
    and "duration" [s ms us ns; a constant also D, or None: NumPy's generic timedelta, which an integer literal is too].
      * T +- duration, duration + T -> T[finer unit] (date +- whole days stays date32); T - T -> duration[finer] (D - D: seconds, Arrow
        has no duration in days); duration +- duration, -duration -> duration[finer]; duration * integer literal -> duration;
        T +- integer literal -> T (the literal in T's own unit);
      * duration / duration -> ("div", a, b) over both sides aligned to the finer unit: float64 in the interpreter, NaT reads as NaN;
        duration // duration -> an int64 column with validity (keydict.floordiv_column: vnm_temporal_floordiv, the factors inside);
      * an int32 / int64 COLUMN under + / - is a generic timedelta too (NumPy casts the integer array to the other operand's unit);
      * constants among themselves fold with NumPy itself; a column against a constant uses c, two columns both factors; a constant
        that does not fit int64 in the unit it is aligned to raises OverflowError;
      * T + T, T * x, T / x, -T, n - T, duration - T, duration * float, duration / number, duration // number, anything with a float
        or a string column, an integer column outside + -: TypeError naming the operator and the operand types; duration % duration:
        NotImplementedError.
    The result is a derived column in `extra` named __temporal_affine..., cached by (operands, factors), or a constant.
    `lower` lowers an operand (the caller's own recursion); an arithmetic node without a temporal operand passes through.
      * is_busday(x[, weekmask[, holidays]]) -> ("ne", mask column, 0) (keydict.busday_mask); x a date32 column or a node that lowers
        to one; a timestamp or string column raises TypeError advising is_busday(date(x));
      * an IN list of temporal constants: column and members aligned to the finest unit among them, the members plain integers."""

    def __init__(self, columns, extra, lower, types_only=False):
        """types_only: plan time (check_temporal) -- the columns are known by their types alone, a result is a column of its type
        and no kernel runs"""
        self.columns, self.extra, self.lower, self.types_only = columns, extra, lower, types_only

    def kind_of(self, x):
        """("temporal" | "duration", unit) of a constant or of a date32 / timestamp / duration column (derived ones included); None for
        anything else"""
        if is_temporal_const(x):
            return x[0], x[2]
        cols = with_derived(self.columns, self.extra)
        if isinstance(x, str) and x in cols and cols[x].dictionary is None:
            t = cols[x].arrow_type
            if K.temporal_unit(t) is not None:
                return "temporal", K.temporal_unit(t)
            if K.duration_unit(t) is not None:
                return "duration", K.duration_unit(t)
        return None

    def describe(self, x) -> str:
        k = self.kind_of(x)
        if k is not None:
            name = "datetime64" if k[0] == "temporal" else "timedelta64"
            return f"{name}[{k[1]}]" if k[1] else name
        cols = with_derived(self.columns, self.extra)
        if isinstance(x, str) and x in cols:
            c = cols[x]
            return f"the {value_type_of(c.dictionary) if c.dictionary is not None else c.arrow_type} column {x!r}"
        if isinstance(x, (int, float)) or (isinstance(x, tuple) and x and x[0] == "strong"):
            v = x[1] if isinstance(x, tuple) else x
            return type(v).__name__
        return f"the expression {x!r}"

    def _column(self, a, ka, b, kb, c, t):
        """the derived column a * ka + b * kb + c of type t (b may be None); a column times 1 of its own type is itself"""
        cols = with_derived(self.columns, self.extra)
        if b is None and ka == 1 and c == 0 and cols[a].arrow_type == t:
            return a
        name = f"{_DERIVED_TEMPORAL}affine({a}*{ka}" + (f"+{b}*{kb}" if b is not None else "") + f"+{c})[{t}]"
        if name not in self.extra:
            self.extra[name] = _Typed(t) if self.types_only else K.affine_column(cols[a], ka, cols[b] if b is not None else None, kb, c, t)
        return name

    def _is_int_column(self, x) -> bool:
        """an int32 / int64 column: the widths vnm_temporal_affine reads"""
        cols = with_derived(self.columns, self.extra)
        return isinstance(x, str) and x in cols and cols[x].dictionary is None and (pa.types.is_int32(cols[x].arrow_type) or pa.types.is_int64(cols[x].arrow_type))

    @staticmethod
    def _scaled(x, have, want):
        v = x[1] * (K.UNITS_PER_DAY[want] // K.UNITS_PER_DAY[have or want])
        if not -2**63 <= v < 2**63:
            raise OverflowError(f"the temporal constant {x[1]} [{have}] does not fit int64 in the unit {want!r} of the other operand")
        return v

    def _binary(self, op, a, b):
        bad = TypeError(f"{op}() cannot use operands with types {self.describe(a)} and {self.describe(b)}")
        ka, kb = self.kind_of(a), self.kind_of(b)
        if ka is None and kb is None:
            return (op, a, b)
        if op == "mul":
            x, n = (a, b) if ka else (b, a)
            if not (self.kind_of(x)[0] == "duration" and _is_int(n)):
                raise bad
            n = n[1] if isinstance(n, tuple) else n
            if is_temporal_const(x):
                return E.temporal_const(E.temporal_scalar(x) * np.int64(n))
            return self._column(x, n, None, 0, 0, pa.duration(self.kind_of(x)[1]))
        if op in ("add", "sub"):
            # an integer literal is NumPy's generic timedelta: it takes the unit of the operand it meets
            if ka is None and _is_int(a):
                a, ka = ("duration", a[1] if isinstance(a, tuple) else a, None), ("duration", None)
            if kb is None and _is_int(b):
                b, kb = ("duration", b[1] if isinstance(b, tuple) else b, None), ("duration", None)
            # ... and so is an int32 / int64 COLUMN (NumPy casts the integer array to timedelta64 of the other operand's unit)
            if ka is None and self._is_int_column(a) and kb[1] is not None:
                ka = ("duration", None)
            if kb is None and self._is_int_column(b) and ka is not None and ka[1] is not None:
                kb = ("duration", None)
        if ka is None or kb is None:
            raise bad
        kinds = (ka[0], kb[0])
        if op == "floordiv":
            if kinds != ("duration", "duration"):
                raise bad
            if is_temporal_const(a) and is_temporal_const(b):
                return ("strong", int(np.floor_divide(E.temporal_scalar(a), E.temporal_scalar(b))))
            want = max((u for u in (ka[1], kb[1]) if u is not None), key=K.TEMPORAL_UNITS.index)
            if want == "D":
                want = "s"
            fa, fb = (K.UNITS_PER_DAY[want] // K.UNITS_PER_DAY[u or want] for u in (ka[1], kb[1]))
            ca, cb = (None, self._scaled(a, ka[1], want)) if is_temporal_const(a) else (a, fa), (None, self._scaled(b, kb[1], want)) if is_temporal_const(b) else (b, fb)
            name = f"{_DERIVED_TEMPORAL}floordiv({ca[0]}*{ca[1]},{cb[0]}*{cb[1]})"
            if name not in self.extra:
                cols = with_derived(self.columns, self.extra)
                self.extra[name] = _Typed(pa.int64()) if self.types_only else \
                    K.floordiv_column(cols[ca[0]] if ca[0] is not None else None, ca[1], cols[cb[0]] if cb[0] is not None else None, cb[1])
            return name
        if op == "div":
            if kinds != ("duration", "duration"):
                raise bad
            out_kind = None
        elif op == "add":
            if kinds == ("temporal", "temporal"):
                raise bad
            out_kind = "temporal" if "temporal" in kinds else "duration"
        elif op == "sub":
            if kinds == ("duration", "temporal"):
                raise bad
            out_kind = "duration" if kinds[0] == kinds[1] else "temporal"
        elif op == "mod" and kinds == ("duration", "duration"):
            raise NotImplementedError("no GPU lowering for duration % duration")
        else:
            raise bad
        if is_temporal_const(a) and is_temporal_const(b):
            v = {"add": np.add, "sub": np.subtract, "div": np.divide}[op](E.temporal_scalar(a), E.temporal_scalar(b))
            return ("strong", float(v)) if op == "div" else E.temporal_const(v)
        units = [u for u in (ka[1], kb[1]) if u is not None]
        want = max(units, key=K.TEMPORAL_UNITS.index)
        if want == "D" and out_kind != "temporal":
            want = "s"                       # (a difference of dates: Arrow has no duration in days)
        fa, fb = (K.UNITS_PER_DAY[want] // K.UNITS_PER_DAY[u or want] for u in (ka[1], kb[1]))
        if op == "div":
            side = lambda x, k, fk: ("strong", self._scaled(x, k[1], want)) if is_temporal_const(x) else self._column(x, fk, None, 0, 0, pa.duration(want))
            return ("div", side(a, ka, fa), side(b, kb, fb))
        t = K.temporal_type(want) if out_kind == "temporal" else pa.duration(want)
        sign = -1 if op == "sub" else 1
        if is_temporal_const(b):
            return self._column(a, fa, None, 0, sign * self._scaled(b, kb[1], want), t)
        if is_temporal_const(a):
            return self._column(b, sign * fb, None, 0, self._scaled(a, ka[1], want), t)
        return self._column(a, fa, b, sign * fb, 0, t)

    def arithmetic(self, e):
        op = E.TEMPORAL_ARITH[e[0]]
        xs = [self.lower(x) for x in e[1:]]
        if not any(self.kind_of(x) for x in xs):
            return E.with_operands(e, xs)
        if op == "neg":
            (x,), k = xs, self.kind_of(xs[0])
            if k[0] != "duration":
                raise TypeError(f"neg() cannot use an operand with type {self.describe(x)}")
            if is_temporal_const(x):
                return E.temporal_const(-E.temporal_scalar(x))
            return self._column(x, -1, None, 0, 0, pa.duration(k[1]))
        acc = xs[0]
        for y in xs[1:]:                   # an n-ary chain folds left, as every operator does
            acc = self._binary(op, acc, y)
        return acc

    def is_busday(self, e):
        if not 2 <= len(e) <= 4:
            raise NotImplementedError(f"no GPU lowering for is_busday() with {len(e) - 1} operand(s)")
        x = self.lower(e[1])
        cols = with_derived(self.columns, self.extra)
        if not isinstance(x, str) or x not in cols:
            raise NotImplementedError(f"no GPU lowering for is_busday() over {x!r}: the operand must be a date32 column or date() of a column")
        c = cols[x]
        if c.dictionary is not None or not pa.types.is_date32(c.arrow_type):
            raise TypeError(f"is_busday() takes a date32 column, {x!r} is {value_type_of(c.dictionary) if c.dictionary is not None else c.arrow_type}: "
                            f"write is_busday(date({x}))")
        weekmask, holidays = busday_arguments(e)
        # keyed on the NORMALISED calendar, as keydict's cache is (ValueError for a spelling NumPy refuses or a list too long)
        bits, days = K.busday_key(weekmask, holidays)
        name = f"__busday({x},{bits:07b},{len(days) // 4}:{hashlib.sha256(days).hexdigest()})"
        if name not in self.extra:
            self.extra[name] =_Typed(pa.uint8()) if self.types_only else K.busday_mask(c, weekmask, holidays)
        return ("ne", name, 0)

    def in_list(self, e, rescale):
        """rescale: the caller's lowering of a ("datetime", column, ("lit", unit)) node"""
        x = self.lower(e[1])
        members = [E.fold_temporal(m) if isinstance(m, tuple) and m and m[0] in TEMPORAL_FNS else m for m in e[2]]
        k = self.kind_of(x)
        if not any(is_temporal_const(m) for m in members):       # a list of plain numbers: the storage integers, as it has always been
            return None if x is e[1] else (e[0], x, e[2])
        what = e[0].upper().replace("_", " ")
        if k is None or k[0] != "temporal":
            raise TypeError(f"{what} with temporal constants over {self.describe(x)}: only a date32 / timestamp column or date() / datetime() / "
                            "from_timestamp() of a column")
        for m in members:
            if not (is_temporal_const(m) and m[0] == "temporal"):
                raise TypeError(f"{what} over {self.describe(x)} needs date() / datetime() / from_timestamp() constants, got {m!r}")
        want = max([k[1]] + [m[2] for m in members], key=K.TEMPORAL_UNITS.index)
        if want != k[1]:
            x = rescale(("datetime", x, ("lit", want)))
        return (e[0], x, tuple(self._scaled(m, m[2], want) for m in members))


def busday_arguments(e):
    """(weekmask, holidays) of an is_busday node as keydict.busday_calendar takes them: the weekmask string or None, the holidays a
    tuple of date strings.  Anything but a string literal / a list of them raises TypeError."""
    text = lambda v: v.decode("utf-8") if isinstance(v, bytes) else v
    weekmask = None
    if len(e) > 2:
        if not E.is_str_lit(e[2]):
            raise TypeError(f"is_busday(): the weekmask must be a string literal ('1111100' or 'Mon Tue ...'), not {e[2]!r}")
        weekmask = text(e[2][1])
    holidays = ()
    if len(e) > 3:
        if not isinstance(e[3], (list, tuple)) or E.is_str_lit(e[3]) or not all(isinstance(h, (str, bytes)) or E.is_str_lit(h) for h in e[3]):
            raise TypeError(f"is_busday(): the holidays must be a list literal of date strings, not {e[3]!r}")
        holidays = tuple(text(h[1] if E.is_str_lit(h) else h) for h in e[3])
    return weekmask, holidays


class _Typed:
    """a column known by its Arrow type alone (plan time); `dictionary` is set for a string / binary column"""

    def __init__(self, t, coded=False):
        self.arrow_type = self.type = t
        self.dictionary = _Typed(t) if coded else None


def check_temporal(expr, types):
    """Plan time: TemporalArithmetic's rules over a schema (types: column name -> Arrow type), no device.  Raises what the lowering
    would raise per batch -- TypeError for operands NumPy refuses, ValueError for a timedelta unit or a holiday list, OverflowError,
    NotImplementedError -- and returns the type-only form of `expr`; what it does not know passes through."""
    columns = {n: _Typed(t, coded=K.device_value_type(t) is not None) for n, t in types.items()}
    extra = {}
    lower = lambda x: E.rewrite(x, f) if isinstance(x, tuple) else x

    def derived(e):
        const = E.fold_temporal(e)
        if const is not None:
            return const
        unit, x = E.temporal_unit_arg(e) or "s", lower(e[1])
        name = f"{_DERIVED_TEMPORAL}{e[0]}_{unit}_{x}"
        extra[name] = _Typed(K.temporal_type(unit))
        return name
    rules = TemporalArithmetic(columns, extra, lower, types_only=True)

    def f(e):
        if e[0] in TEMPORAL_FNS:
            return derived(e)
        if e[0] == "timedelta":
            return E.fold_timedelta(e)
        if e[0] in E.TEMPORAL_ARITH:
            return rules.arithmetic(e)
        if e[0] == "is_busday":
            return rules.is_busday(e)
        if e[0] in E.IN_OPS and len(e) == 3:
            return rules.in_list(e, derived)
        return None
    return lower(expr)


def lower_like(expr, columns, extra=None):
    """LIKE / NOT LIKE (LikeFunction, vinum/core/functions.py:301-344) -> a lookup in a per-pattern table of the column's
    dictionary: ("like", col, ("lit", p)) becomes ("lookup", col, table) and ("not_like", ...) ("not", ("lookup", ...)), where
    `table` names a uint8 column added to `extra` (KeyDictionary.like_table: one byte per dictionary id, matched on the device
    once per distinct value).  A NULL row looks up 0: LIKE is false, NOT LIKE true -- the project's rule for `=` / `!=`.
    Only a utf8 / large_utf8 column and a string literal pattern lower; other column types raise TypeError as in the
    reference, other shapes NotImplementedError."""
    extra = {} if extra is None else extra

    def f(e):
        if e[0] not in ("like", "not_like"):
            return None
        if len(e) != 3:
            raise NotImplementedError(f"no GPU lowering for a {e[0].upper()} node with {len(e) - 1} operand(s)")
        col, pat = e[1], e[2]
        if not (E.is_str_lit(pat) and isinstance(pat[1], str)):
            raise NotImplementedError(f"no GPU lowering for {e[0].upper()} with the pattern {pat!r}: a string literal is required")
        if not isinstance(col, str) or col not in columns:
            raise NotImplementedError(f"no GPU lowering for {e[0].upper()} over {col!r}: the operand must be a column")
        c = columns[col]
        if c.dictionary is None:
            raise TypeError(f"LIKE needs a string column, {col!r} is {c.arrow_type}")
        name = f"__like_{len(extra)}_{col}"
        extra[name] = c.dictionary.like_table(pat[1])
        node = ("lookup", col, name)
        return node if e[0] == "like" else ("not", node)
    return E.rewrite(expr, f), extra


# the arithmetic, bitwise, math and cast operators of ops.compile_expr: what takes a NUMBER, which a dictionary code is not
_ARITHMETIC = ("add", "sub", "mul", "div", "mod", "neg", "+", "-", "*", "/", "%", "band", "bor", "bxor", "bnot", "abs", "sqrt", "sin",
               "cos", "tan", "log", "log2", "log10", "power", "to_float", "to_int", "to_bool")


def lower_column_compares(expr, columns, extra=None):
    """Comparisons of a dictionary-coded column with ANOTHER such column -- `city_from = city_to`, `city_from < city_to`; the
    reference compares the two value arrays, vinum/core/expressions.py:30-36.  The codes of two dictionaries mean nothing to each
    other, so:
      * both columns share one dictionary object: = / != stay as they are (equal codes <=> equal values), the ordered operators
        compare the two columns' ranks (KeyDictionary.rank_column);
      * otherwise = / != become (op, a, ("lookup_i32", b, table)) with b's codes translated into a's
        (KeyDictionary.translate_table: -2 where a's dictionary does not hold the value), and < <= > >= become
        (op, ("lookup_i32", a, ranks_a), ("lookup_i32", b, ranks_b)) with the ranks of both dictionaries in the byte order of
        their union (KeyDictionary.joint_rank_tables).
    BETWEEN / NOT BETWEEN with a dictionary-coded operand is rewritten onto >= <= / < > first (expr.desugar does it too late for
    this lowering), so column bounds follow.  Bytes are compared exactly, as a literal's are (no trailing-NUL rule); utf8,
    large_utf8, binary and large_binary mix freely.  A NULL on either side compares False, `!=` True.
    What has no meaning raises instead of comparing codes: a dictionary-coded column against a numeric column, literal or
    expression, IN / NOT IN over one with a list that is not all string / binary literals, and one as the operand of an
    arithmetic, bitwise, math or cast operator (_ARITHMETIC: TypeError); a pair with a host-route dictionary -- bool, decimal,
    date64 -- (NotImplementedError).  Any other operator over such a column (a string function, say) passes through untouched
    and is accepted or refused where it is compiled."""
    extra = {} if extra is None else extra

    def rank_name(c):
        name = f"__rank_{c}"
        if name not in extra:
            extra[name] = columns[c].dictionary.rank_column(columns[c])
        return name

    def f(e):
        op = E.cmp_name(e[0])
        if e[0] in ("between", "not_between") and len(e) == 4 and any(_is_dict(x, columns) for x in e[1:]):
            x, lo, hi = e[1:]
            return E.rewrite(("and", ("ge", x, lo), ("le", x, hi)) if e[0] == "between" else ("or", ("lt", x, lo), ("gt", x, hi)), f)
        if op and len(e) == 3:
            a, b = e[1], e[2]
            if _is_dict(a, columns) and _is_dict(b, columns):
                da, db = columns[a].dictionary, columns[b].dictionary
                if da is db:
                    return e if op in ("eq", "ne") else (op, rank_name(a), rank_name(b))
                if not (getattr(da, "on_device", False) and getattr(db, "on_device", False)):
                    raise NotImplementedError(f"no GPU lowering for comparing {a!r} ({value_type_of(da)}) with {b!r} ({value_type_of(db)}): only string "
                                              "and binary columns keep their dictionaries on the device")
                if op in ("eq", "ne"):
                    name = f"__codes_of_{b}_in_{a}"
                    if name not in extra:
                        extra[name] = db.translate_table(da)
                    return (op, a, ("lookup_i32", b, name))
                na, nb = f"__joint_rank_{a}_with_{b}", f"__joint_rank_{b}_with_{a}"
                if na not in extra:
                    extra[na], extra[nb] = da.joint_rank_tables(db)
                return (op, ("lookup_i32", a, na), ("lookup_i32", b, nb))
            for x, y in ((a, b), (b, a)):
                if _is_dict(x, columns) and not E.is_str_lit(y):
                    raise TypeError(f"cannot compare the {value_type_of(columns[x].dictionary)} column {x!r} with {y!r}: only a string / "
                                    "binary literal or another such column")
        elif e[0] in _ARITHMETIC:
            for x in e[1:]:
                if _is_dict(x, columns):
                    raise TypeError(f"{e[0]}() over the {value_type_of(columns[x].dictionary)} column {x!r}: not a numeric operand")
        elif e[0] in E.IN_OPS and _is_dict(e[1], columns) and not all(isinstance(v, (str, bytes)) or E.is_str_lit(v) for v in e[2]):
            raise TypeError(f"{e[0].upper().replace('_', ' ')} over the {value_type_of(columns[e[1]].dictionary)} column {e[1]!r} needs string / "
                            f"binary literals, got {list(e[2])!r}")
        return None
    return E.rewrite(expr, f), extra


def lower_literal_compares(expr, columns, extra=None):
    """Comparisons of a dictionary-coded column with a LITERAL -- `city = 'Berlin'`, `name < 'M'`, `city IN ('a', 'b')`, in either
    spelling of the operator and either operand order -- become numeric comparisons: = / != / IN on the literal's CODE (a value the
    dictionary does not hold matches no row), < <= > >= on the column's order-preserving RANKS (KeyDictionary.rank_column:
    byte-wise order, as Arrow / NumPy compare such values) against the literal's position among the dictionary's values.  NULL rows
    behave as in every other predicate (compare False, `!=` True: vinum/arrow/record_batch.py:112-118).  An IN list's codes are an
    int64 list over an int32 column: a long one is probed as a set like any numeric list (ops.lower_in_sets), per batch, because the
    dictionary grows."""
    extra = {} if extra is None else extra

    def f(e):
        op = E.cmp_name(e[0])
        if op and len(e) == 3:
            a, b = e[1], e[2]
            if E.is_str_lit(a) and _is_dict(b, columns):
                a, b, op = b, a, E.CMP_FLIP[op]
            if _is_dict(a, columns) and E.is_str_lit(b):
                d = columns[a].dictionary
                if op in ("eq", "ne"):
                    c = d.code_of(b[1])
                    return (op, a, -2 if c is None else c)            # (codes are >= 0)
                name = f"__rank_{a}"
                if name not in extra:
                    extra[name] = d.rank_column(columns[a])
                less, present = d.rank_bounds(b[1])
                return {"lt": ("lt", name, less), "le": ("lt", name, less + present),
                        "gt": ("ge", name, less + present), "ge": ("ge", name, less)}[op]
        if e[0] in E.IN_OPS and _is_dict(e[1], columns) and all(isinstance(v, (str, bytes)) or E.is_str_lit(v) for v in e[2]):
            d = columns[e[1]].dictionary
            codes = [d.code_of(v[1] if E.is_str_lit(v) else v) for v in e[2]]
            return (e[0], e[1], tuple(c for c in codes if c is not None) or (-2,))
        return None
    return E.rewrite(expr, f), extra


def lower_dictionary(expr, columns, extra=None):
    """The four lowerings in their order: upper() / lower() / concat() / to_str() -- whose results are string columns to the other three -- and
    date() / datetime() / from_timestamp() -- whose results are temporal columns --, LIKE, then
    the column pairs -- which refuse a numeric operand, so they run before the literals turn into codes and ranks -- then the
    literals; the last two only act where a dictionary-coded column is read at all."""
    expr, extra = lower_case_functions(expr, columns, extra)
    columns = with_derived(columns, extra)
    expr, extra = lower_like(expr, columns, extra)
    if any(_is_dict(c, columns) for c in E.columns_of(expr)):
        expr, extra = lower_column_compares(expr, columns, extra)
        expr, extra = lower_literal_compares(expr, columns, extra)
    return expr, extra


def used_columns(exprs, columns, extra):
    """name -> column of everything the lowered `exprs` read, in first-use order: from `extra` where a lowering made it"""
    return {c: extra[c] if c in extra else columns[c] for e in exprs for c in E.columns_of(e)}


def project_lowered(exprs, columns, length, scalar_length=None):
    """ops.project_many of `exprs` lowered into one shared `extra`; scalar_length: the length when none of them reads a column.
    An expression that lowers to a column -- upper(city): the derived column of `extra`; datetime(ts, 'ms') over a timestamp[ms] column:
    the input column itself -- is that column, no program runs."""
    extra = {}
    exprs = [lower_dictionary(e, columns, extra)[0] for e in exprs]
    column_of = lambda e: extra[e] if e in extra else columns[e]
    is_column = lambda e: isinstance(e, str) and (e in extra or e in columns)
    computed = [e for e in exprs if not is_column(e)]
    used = used_columns(computed, columns, extra)
    res = iter(ops.project_many(computed, used, length=length if used or scalar_length is None else scalar_length) if computed else [])
    return [column_of(e) if is_column(e) else next(res) for e in exprs]
