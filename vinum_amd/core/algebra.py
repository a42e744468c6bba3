"""GPU counterparts of the reference's Python physical operators (vinum/core/algebra.py)."""
from typing import Optional, Sequence, Tuple

import pyarrow as pa

from .. import expr as E
from .. import get_batch_size, ops
from ..device import is_supported
from .base import DeviceRecordBatch, Operator
from .lowering import lower_column_compares, lower_dictionary, project_lowered, used_columns, value_type_of  # noqa: F401 (see FilterOperator)


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


class FilterOperator(Operator):
    """algebra.py:108-123: `WHERE column <op> literal`; every column of the batch is compacted (no selection
    vectors in the reference either).  predicate = (column, op, literal)."""

    def __init__(self, predicate: Tuple[str, str, object], parent_operator: Operator):
        super().__init__(parent_operator)
        self.predicate = predicate

    # lower_dictionary over a BATCH; with lower_column_compares above, the two old names test_strcmp_cpu.py / test_gpu_strcmp.py use
    lower_dictionary_predicates = staticmethod(lambda pred, batch, extra=None: lower_dictionary(pred, batch.columns, extra))

    @staticmethod
    def is_simple(pred) -> bool:
        """`column <op> literal`: the shape that runs fused (and can be folded into an aggregate scan)."""
        return (isinstance(pred, tuple) and len(pred) == 3 and isinstance(pred[0], str) and pred[1] in ops.CMP_OPS
                and isinstance(pred[2], (int, float)) and not isinstance(pred[2], bool))

    def _kernel(self, batch: DeviceRecordBatch) -> DeviceRecordBatch:
        names = batch.column_names
        cols = [batch.columns[n] for n in names]
        pred = self.predicate
        if self.is_simple(pred) or (isinstance(pred, tuple) and len(pred) == 3 and pred[1] in E.CMP_SYMBOL.values()
                                    and isinstance(pred[2], (str, bytes))):
            col, op, lit = pred
            if isinstance(lit, (str, bytes)):       # (column, "==", "Berlin") over a dictionary-coded column
                pred = (E.cmp_name(op), col, ("lit", lit))
            else:
                if batch.column(col).dictionary is not None:
                    raise TypeError(f"cannot compare the {value_type_of(batch.column(col).dictionary)} column {col!r} with {lit!r}: only a "
                                    "string / binary literal or another such column")
                outs, k = ops.filter_cmp(batch.column(col), op, lit, cols)
                return DeviceRecordBatch(dict(zip(names, outs)), k)
        # general boolean expression tree: the dictionary lowerings (core.lowering), one fused mask kernel, one compaction pass
        pred, extra = lower_dictionary(pred, batch.columns)
        mask = ops.predicate_mask(pred, used_columns([pred], batch.columns, extra), batch.num_rows)
        outs, k = ops.filter_mask(mask, None, batch.num_rows, cols)
        return DeviceRecordBatch(dict(zip(names, outs)), k)


class ProjectOperator(Operator):
    """algebra.py:28-105: expressions (prefix tuples, see vinum_amd.expr) or plain column names -> output columns.
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
        # every computed expression of the SELECT list goes into one fused kernel, lowered first (core.lowering; a predicate keeps
        # the uint8 mask result type); column-free expressions repeat their scalar once per row (:77-87)
        named = [(name, arg) for name, arg in zip(self._col_names, self._arguments) if not isinstance(arg, str)]
        res = project_lowered([e for _, e in named], batch.columns, n, scalar_length=max(n, 1)) if named else []
        computed = {name: col for (name, _), col in zip(named, res)}
        for name, arg in zip(self._col_names, self._arguments):
            out[name] = batch.column(arg) if isinstance(arg, str) else computed[name]
        return DeviceRecordBatch(out, n)


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
