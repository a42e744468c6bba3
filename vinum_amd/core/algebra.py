"""GPU counterparts of the reference's Python physical operators (vinum/core/algebra.py)."""
from typing import Iterable, List, Optional, Sequence, Tuple

import pyarrow as pa

from .. import get_batch_size, ops
from .. import _lib as L
from ..device import DeviceColumn, is_supported
from .base import DeviceRecordBatch, Operator


class TableReaderOperator(Operator):
    """algebra.py:250-265 + table_batch_reader.cpp: slices the table into batches of vinum_amd.get_batch_size() rows
    (2^24 by default -- the reference's 10 000 would mean 1e5 launches per 1e9 rows) and stages them into HBM.
    `columns` prunes what is staged (the planner's pruning projection, planner.py:367-371)."""

    def __init__(self, table: pa.Table, columns: Optional[Sequence[str]] = None):
        super().__init__(None)
        self._table = table.select(list(columns)) if columns is not None else table
        self._dicts = {}     # running dictionaries of the non-numeric columns (shared by every batch of this scan)

    def next(self):
        for b in self._table.to_batches(max_chunksize=get_batch_size()):
            yield DeviceRecordBatch.from_arrow(b, self._dicts)


class FileReaderOperator(Operator):
    """algebra.py:268-279: pulls from a pyarrow streaming reader (pyarrow.csv.open_csv, io/arrow.py:58-61) until
    StopIteration.  Only GPU-representable columns are staged."""

    def __init__(self, reader, columns: Optional[Sequence[str]] = None):
        super().__init__(None)
        self._reader, self._columns = reader, columns
        self._dicts = {}

    def next(self):
        while True:
            if hasattr(self._reader, "read_next_device_batch"):     # vinum_amd.io.GpuCsvReader: columns are born in HBM
                try:
                    yield self._reader.read_next_device_batch()
                except StopIteration:
                    break
                continue
            try:
                batch = self._reader.read_next_batch()
            except StopIteration:
                break
            names = self._columns if self._columns is not None else [f.name for f in batch.schema if is_supported(f.type)]
            yield DeviceRecordBatch.from_arrow(batch.select(list(names)), self._dicts)


def lower_like(expr, columns, extra=None):
    """LIKE / NOT LIKE (LikeFunction, vinum/core/functions.py:301-344) -> a lookup in a per-pattern table of the column's
    dictionary: ("like", col, ("lit", p)) becomes ("lookup", col, table) and ("not_like", ...) ("not", ("lookup", ...)), where
    `table` names a uint8 column added to `extra` (KeyDictionary.like_table: one byte per dictionary id, matched on the device
    once per distinct value).  A NULL row looks up 0: LIKE is false, NOT LIKE true -- the project's rule for `=` / `!=`.
    Only a utf8 / large_utf8 column and a string literal pattern lower; other column types raise TypeError as in the
    reference, other shapes NotImplementedError.  Returns (expression, extra)."""
    extra = {} if extra is None else extra

    def walk(e):
        if not isinstance(e, tuple) or not e or e[0] == "lit":
            return e
        if e[0] in ("like", "not_like"):
            if len(e) != 3:
                raise NotImplementedError(f"no GPU lowering for a {e[0].upper()} node with {len(e) - 1} operand(s)")
            col, pat = e[1], e[2]
            if not (isinstance(pat, tuple) and len(pat) == 2 and pat[0] == "lit" and isinstance(pat[1], str)):
                raise NotImplementedError(f"no GPU lowering for {e[0].upper()} with the pattern {pat!r}: a string literal is required")
            if not isinstance(col, str) or col not in columns:
                raise NotImplementedError(f"no GPU lowering for {e[0].upper()} over {col!r}: the operand must be a column")
            c = columns[col]
            if c.dictionary is None:
                raise TypeError(f"LIKE needs a string column, {col!r} is {c.arrow_type}")
            table = c.dictionary.like_table(pat[1])
            name = f"__like_{len(extra)}_{col}"
            extra[name] = table
            node = ("lookup", col, name)
            return node if e[0] == "like" else ("not", node)
        if e[0] in ("in", "not_in"):
            return (e[0], walk(e[1]), e[2])
        return tuple([e[0]] + [walk(x) for x in e[1:]])
    return walk(expr), extra


_CMP = ("eq", "ne", "lt", "le", "gt", "ge")
_CMP_NAME = {"==": "eq", "=": "eq", "!=": "ne", "<>": "ne", ">": "gt", ">=": "ge", "<": "lt", "<=": "le"}
# the arithmetic, bitwise, math and cast operators of ops.compile_expr: what takes a NUMBER, which a dictionary code is not
_ARITHMETIC = ("add", "sub", "mul", "div", "mod", "neg", "+", "-", "*", "/", "%", "band", "bor", "bxor", "bnot", "abs", "sqrt", "sin",
               "cos", "tan", "log", "log2", "log10", "power", "to_float", "to_int", "to_bool")


def lower_column_compares(expr, columns, extra=None):
    """Comparisons of a dictionary-coded column (strings, binaries: int32 codes of the column's OWN running dictionary) with
    ANOTHER such column -- `city_from = city_to`, `city_from < city_to`; the reference compares the two value arrays,
    vinum/core/expressions.py:30-36.  The codes of two dictionaries mean nothing to each other, so:
      * both columns share one dictionary object: = / != stay as they are (equal codes <=> equal values), the ordered operators
        compare the two columns' ranks (KeyDictionary.rank_column);
      * otherwise = / != become (op, a, ("lookup_i32", b, table)) with b's codes translated into a's
        (KeyDictionary.translate_table: -2 where a's dictionary does not hold the value), and < <= > >= become
        (op, ("lookup_i32", a, ranks_a), ("lookup_i32", b, ranks_b)) with the ranks of both dictionaries in the byte order of
        their union (KeyDictionary.joint_rank_tables).
    BETWEEN / NOT BETWEEN with a dictionary-coded operand is rewritten onto >= <= / < > first (ops._desugar does it too late for
    this lowering), so column bounds follow.  Bytes are compared exactly, as a literal's are (no trailing-NUL rule); utf8,
    large_utf8, binary and large_binary mix freely.  A NULL on either side compares False, `!=` True.
    What has no meaning raises instead of comparing codes: a dictionary-coded column against a numeric column, literal or
    expression, IN / NOT IN over one with a list that is not all string / binary literals, and one as the operand of an
    arithmetic, bitwise, math or cast operator (_ARITHMETIC: TypeError); a pair with a host-route dictionary -- bool, decimal,
    date64 -- (NotImplementedError).  Any other operator over such a column (a string function, say) passes through untouched
    and is accepted or refused where it is compiled.  Tables and rank columns are added to `extra`.  Returns (expression, extra)."""
    extra = {} if extra is None else extra

    def is_dict(x):
        return isinstance(x, str) and x in columns and columns[x].dictionary is not None

    def is_str_lit(x):
        return isinstance(x, tuple) and len(x) == 2 and x[0] == "lit" and isinstance(x[1], (str, bytes))

    def rank_name(c):
        name = f"__rank_{c}"
        if name not in extra:
            extra[name] = columns[c].dictionary.rank_column(columns[c])
        return name

    def walk(e):
        if not isinstance(e, tuple) or not e or e[0] in ("lit", "strong"):
            return e
        op = _CMP_NAME.get(e[0], e[0])
        if op in ("between", "not_between") and len(e) == 4 and any(is_dict(x) for x in e[1:]):
            x, lo, hi = e[1:]
            return walk(("and", ("ge", x, lo), ("le", x, hi)) if op == "between" else ("or", ("lt", x, lo), ("gt", x, hi)))
        if op in _CMP and len(e) == 3:
            a, b = e[1], e[2]
            if is_dict(a) and is_dict(b):
                da, db = columns[a].dictionary, columns[b].dictionary
                if da is db:
                    return e if op in ("eq", "ne") else (op, rank_name(a), rank_name(b))
                if not (getattr(da, "on_device", False) and getattr(db, "on_device", False)):
                    raise NotImplementedError(f"no GPU lowering for comparing {a!r} ({da.type}) with {b!r} ({db.type}): only string "
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
                if is_dict(x) and not is_str_lit(y):
                    raise TypeError(f"cannot compare the {columns[x].dictionary.type} column {x!r} with {y!r}: only a string / "
                                    "binary literal or another such column")
        elif op in _ARITHMETIC:
            for x in e[1:]:
                if is_dict(x):
                    raise TypeError(f"{op}() over the {columns[x].dictionary.type} column {x!r}: not a numeric operand")
        if op in ("in", "not_in"):
            if is_dict(e[1]) and not all(isinstance(v, (str, bytes)) or is_str_lit(v) for v in e[2]):
                raise TypeError(f"{op.upper().replace('_', ' ')} over the {columns[e[1]].dictionary.type} column {e[1]!r} needs string / "
                                f"binary literals, got {list(e[2])!r}")
            return (op, walk(e[1]), e[2])
        return tuple([e[0]] + [walk(x) for x in e[1:]])
    return walk(expr), extra


class FilterOperator(Operator):
    """algebra.py:108-123: `WHERE column <op> literal`; every column of the batch is compacted (no selection
    vectors in the reference either).  predicate = (column, op, literal)."""

    def __init__(self, predicate: Tuple[str, str, object], parent_operator: Operator):
        super().__init__(parent_operator)
        self.predicate = predicate

    @staticmethod
    def is_simple(pred) -> bool:
        """`column <op> literal`: the shape that runs fused (and can be folded into an aggregate scan)."""
        return (isinstance(pred, tuple) and len(pred) == 3 and isinstance(pred[0], str) and pred[1] in ops.CMP_OPS
                and isinstance(pred[2], (int, float)) and not isinstance(pred[2], bool))

    _FLIP = {"lt": "gt", "le": "ge", "gt": "lt", "ge": "le", "eq": "eq", "ne": "ne"}
    _SYM = {"==": "eq", "!=": "ne", ">": "gt", ">=": "ge", "<": "lt", "<=": "le"}

    @classmethod
    def lower_dictionary_predicates(cls, pred, batch: DeviceRecordBatch, extra=None):
        """Comparisons of a dictionary-coded column (strings, binaries: int32 codes in HBM) with a LITERAL -- `city = 'Berlin'`,
        `name < 'M'`, `city IN ('a', 'b')`; literals are ("lit", value) nodes, a bare str is a column name -- become numeric
        comparisons: = / != / IN on the literal's CODE (a value the dictionary does not hold matches no row), < <= > >= on the
        column's order-preserving RANKS (KeyDictionary.rank_column: byte-wise order, as Arrow / NumPy compare such values) against
        the literal's position among the dictionary's values.  NULL rows behave as in every other predicate (compare False,
        `!=` True: vinum/arrow/record_batch.py:112-118).  LIKE / NOT LIKE become lookups in the dictionary's match table
        (lower_like); comparisons with ANOTHER dictionary-coded column lookups of translated codes / joint ranks
        (lower_column_compares, which also raises for a numeric operand).  An IN list's codes are an int64 list over an int32 column: a
        long one is probed as a set like any numeric list (ops.lower_in_sets), per batch, because the dictionary grows.
        Returns (predicate, extra columns the predicate reads); tables are added to `extra` when one is passed in."""
        pred, extra = lower_like(pred, batch.columns, extra)
        pred, extra = lower_column_compares(pred, batch.columns, extra)

        def is_dict(x):
            return isinstance(x, str) and x in batch.columns and batch.columns[x].dictionary is not None

        def is_lit(x):
            return isinstance(x, tuple) and len(x) == 2 and x[0] == "lit" and isinstance(x[1], (str, bytes))

        def walk(e):
            if not isinstance(e, tuple) or not e:
                return e
            op = e[0]
            if op in cls._FLIP and len(e) == 3:
                a, b = e[1], e[2]
                if is_lit(a) and is_dict(b):
                    a, b, op = b, a, cls._FLIP[op]
                if is_dict(a) and is_lit(b):
                    d = batch.columns[a].dictionary
                    if op in ("eq", "ne"):
                        c = d.code_of(b[1])
                        return (op, a, -2 if c is None else c)            # (codes are >= 0)
                    name = f"__rank_{a}"
                    if name not in extra:
                        extra[name] = d.rank_column(batch.columns[a])
                    less, present = d.rank_bounds(b[1])
                    return {"lt": ("lt", name, less), "le": ("lt", name, less + present),
                            "gt": ("ge", name, less + present), "ge": ("ge", name, less)}[op]
            if op in ("in", "not_in") and is_dict(e[1]) and all(isinstance(v, (str, bytes)) or is_lit(v) for v in e[2]):
                d = batch.columns[e[1]].dictionary
                codes = [d.code_of(v[1] if is_lit(v) else v) for v in e[2]]
                return (op, e[1], tuple(c for c in codes if c is not None) or (-2,))
            if op in ("in", "not_in"):
                return (op, walk(e[1]), e[2])
            return tuple([op] + [walk(x) for x in e[1:]])
        return walk(pred), extra

    def _kernel(self, batch: DeviceRecordBatch) -> DeviceRecordBatch:
        names = batch.column_names
        cols = [batch.columns[n] for n in names]
        pred = self.predicate
        if self.is_simple(pred) or (isinstance(pred, tuple) and len(pred) == 3 and pred[1] in self._SYM and isinstance(pred[2], (str, bytes))):
            col, op, lit = pred
            if isinstance(lit, (str, bytes)):       # (column, "==", "Berlin") over a dictionary-coded column
                pred = (self._SYM[op], col, ("lit", lit))
            else:
                if batch.column(col).dictionary is not None:
                    raise TypeError(f"cannot compare the {batch.column(col).dictionary.type} column {col!r} with {lit!r}: only a "
                                    "string / binary literal or another such column")
                outs, k = ops.filter_cmp(batch.column(col), op, lit, cols)
                return DeviceRecordBatch(dict(zip(names, outs)), k)
        pred, extra = self.lower_dictionary_predicates(pred, batch)
        # general boolean expression tree: one fused mask kernel, then one compaction pass
        columns = dict(batch.columns)
        columns.update(extra)
        mask = ops.predicate_mask(pred, columns, batch.num_rows)
        outs, k = ops.filter_mask(mask, None, batch.num_rows, cols)
        return DeviceRecordBatch(dict(zip(names, outs)), k)


class ProjectOperator(Operator):
    """algebra.py:28-105: expressions (prefix tuples, see ops.compile_expr) or plain column names -> output columns.
    keep_input_table appends instead of replacing (:56-62)."""

    def __init__(self, arguments: Sequence, parent_operator: Operator, col_names: Optional[Sequence[str]] = None,
                 keep_input_table: bool = False):
        super().__init__(parent_operator)
        self._arguments = list(arguments)
        self._col_names = list(col_names) if col_names is not None else [a if isinstance(a, str) else f"expr_{i}"
                                                                          for i, a in enumerate(arguments)]
        self._keep = keep_input_table

    def _kernel(self, batch: DeviceRecordBatch) -> DeviceRecordBatch:
        out = dict(batch.columns) if self._keep else {}
        n = batch.num_rows
        # every computed expression of the SELECT list goes into one fused kernel
        exprs, used, extra = [], {}, {}
        for name, arg in zip(self._col_names, self._arguments):
            if not isinstance(arg, str):
                # LIKE nodes and comparisons of two dictionary-coded columns become dictionary lookups, a string literal or list its
                # codes in the column's dictionary (a predicate keeps the uint8 mask result type)
                arg, _ = FilterOperator.lower_dictionary_predicates(arg, batch, extra)
                exprs.append((name, arg))
                for c in _columns_of(arg):
                    used[c] = extra[c] if c in extra else batch.columns[c]
        computed = {}
        if exprs:
            # column-free expressions repeat their scalar once per row (:77-87)
            res = ops.project_many([e for _, e in exprs], used, length=n if used else max(n, 1))
            computed = {name: col for (name, _), col in zip(exprs, res)}
        for name, arg in zip(self._col_names, self._arguments):
            out[name] = batch.column(arg) if isinstance(arg, str) else computed[name]
        return DeviceRecordBatch(out, n if out and any(not isinstance(a, (int, float)) for a in self._arguments) else n)


def _columns_of(expr) -> List[str]:
    return ops.columns_of(expr)


class SortOperator(Operator):
    """algebra.py:126-201 + sort.cpp: buffers every batch, one stable multi-key sort, all columns taken.
    limit > 0 pushes LIMIT into the sort (same rows as sorting everything, then SliceOperator)."""

    def __init__(self, columns: Sequence[str], sort_order: Sequence[int], parent_operator: Operator, limit: int = 0):
        super().__init__(parent_operator)
        self._cols, self._orders, self._limit = list(columns), [int(o) for o in sort_order], int(limit)

    def next(self):
        batches = [b.to_arrow() for b in self._parent_operator.next()]
        if not batches:
            return
        table = pa.Table.from_batches(batches).combine_chunks()       # Table::FromRecordBatches (sort.cpp:16)
        for f in table.schema:
            if f.name in self._cols and pa.types.is_boolean(f.type):   # algebra.py:191-201
                raise RuntimeError("Sorting by boolean column is not supported yet. "
                                   "Please use float(bool_column) as a workaround.")
        dicts = {}
        dev = DeviceRecordBatch.from_arrow(table.to_batches()[0] if table.num_rows else pa.RecordBatch.from_arrays(
            [pa.array([], f.type) for f in table.schema], names=table.schema.names), dicts).columns
        n = table.num_rows
        k = self._limit if 0 < self._limit < n else 0
        m = k if k else n
        # a string / binary / decimal ... sort key is dictionary-coded in HBM: its order-preserving ranks are the key (NULL stays
        # NULL, equal values share a rank -- the stable sort keeps their row order like SortIndices, sort.cpp:22-37)
        keys = [dev[c] if dev[c].dictionary is None else dev[c].dictionary.rank_column(dev[c]) for c in self._cols]
        sorted_key = None
        if k:
            idx = ops.sort_indices(keys, self._orders, limit=k)
        else:   # a full sort hands its first key back sorted: one gather less
            idx, sorted_key = ops.sort_indices_keyed(keys, self._orders)
        if dev[self._cols[0]].dictionary is not None:
            sorted_key = None          # (the sorted ranks are not the column)
        yield DeviceRecordBatch({name: sorted_key if (sorted_key is not None and name == self._cols[0]) else ops.take(col, idx, m)
                                 for name, col in dev.items()}, m)


class SliceOperator(Operator):
    """LIMIT / OFFSET over the batch stream (algebra.py:204-247).  Rows are counted across batches; a batch that is only
    partly wanted is narrowed to a VIEW of the same HBM buffers (Arrow offset + length, as pa.RecordBatch.slice does on
    the host) -- nothing is copied and nothing leaves the device."""

    def __init__(self, limit: int, offset: int, parent_operator: Operator):
        super().__init__(parent_operator)
        self._limit, self._offset = int(limit), int(offset)

    def next(self):
        skip, want = self._offset, self._limit
        for batch in self._parent_operator.next():
            if want <= 0:
                break
            n = batch.num_rows
            if skip >= n:
                skip -= n
                continue
            take = min(want, n - skip)
            yield batch if (skip == 0 and take == n) else batch.slice(skip, take)
            want -= take
            skip = 0


class MaterializeTableOperator(Operator):
    """algebra.py:290-295: pulls everything, returns one pyarrow Table (the only D2H of the pipeline)."""

    def next(self):
        batches = [b.to_arrow() for b in self._parent_operator.next()]
        yield pa.Table.from_batches(batches) if batches else pa.table({})
