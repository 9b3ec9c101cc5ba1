"""Shared pieces of the Extract() tests: the numpy oracle, the filter list
and helpers that run on the host (tests/test_extract.py) and on the device
(tests/test_gpu_extract.py).

A fixture ``d`` is one of tests/distinct_util.py: ``cols`` (every column that
holds a value somewhere), ``vals`` / ``has`` per int field, ``rows`` {row of set
field f: mask over cols}, ``extra`` (columns that exist, sit in row 1 of f and
hold no value in any int field)."""
from __future__ import annotations

import numpy as np


def filters(d, other="w", bound=500):
    """[(filter text, ascending uint64 columns of the filter)]: a plain row (it
    holds the valueless ``extra`` columns too), an intersection, a negation, a
    BSI predicate on another field, a row that does not exist, one column, and
    two rows that share no column."""
    r = d.rows
    return [
        ("Row(f=1)", np.sort(np.concatenate([d.cols[r[1]], d.extra]))),
        ("Intersect(Row(f=1), Row(f=4))", np.sort(d.cols[r[1] & r[4]])),
        ("Not(Row(f=1))", np.sort(d.cols[~r[1]])),
        (f"Row({other} > {bound})", np.sort(d.cols[d.has[other] & (d.vals[other] > bound)])),
        ("Row(f=9)", np.zeros(0, np.uint64)),
        ("Row(f=5)", np.sort(d.cols[r[5]])),
        ("Union(Row(f=2), Row(f=3))", np.sort(d.cols[r[2] | r[3]])),
    ]


def int_cells(d, field, columns):
    """The oracle's value per column of an int field: the value, or None."""
    order = np.argsort(d.cols)
    pos = np.searchsorted(d.cols[order], columns)
    pos = np.minimum(pos, len(d.cols) - 1)
    at = order[pos]
    hit = (d.cols[at] == columns) & d.has[field][at]
    return [int(v) if ok else None for v, ok in zip(d.vals[field][at].tolist(), hit.tolist())]


def window(columns, offset=0, limit=None):
    return columns[offset:] if limit is None else columns[offset:offset + limit]


def call_text(filt, fields, offset=None, limit=None):
    args = [filt] + [f"Rows(field={f})" for f in fields]
    if limit is not None:
        args.append(f"limit={limit}")
    if offset is not None:
        args.append(f"offset={offset}")
    return "Extract(" + ", ".join(args) + ")"


def check_ints(d, table, fields, columns):
    """``table`` holds exactly ``columns`` and the oracle's values of the int
    ``fields`` (which lead the table's fields)."""
    assert table.columns.dtype == np.uint64 and table.columns.tolist() == columns.tolist()
    for i, f in enumerate(fields):
        assert table.fields[i] == (f, "int64")
        vals, valid = table.data[i]
        assert vals.dtype == np.int64 and valid.dtype == bool and len(vals) == len(valid) == len(columns)
        assert table.cells(i) == int_cells(d, f, columns), f
        assert not vals[~valid].any(), "a null carries a value"
