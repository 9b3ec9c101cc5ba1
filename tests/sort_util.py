"""Shared pieces of the Sort() tests: the numpy oracle (np.lexsort by value,
then column), the call text and the cut positions run on the host
(tests/test_sort.py) and on the device (tests/test_gpu_sort.py).

A fixture ``d`` is one of tests/distinct_util.py: ``cols`` (every column that
holds a value somewhere), ``vals`` / ``has`` per int field (real values) and
``rows`` {row of set field f: mask over cols}."""
from __future__ import annotations

import numpy as np


def oracle(d, field, mask, desc=False):
    """(uint64 columns, int64 values) of the considered columns -- those of
    ``mask`` that hold a value in ``field`` -- ordered by value (descending
    with ``desc``), ties by column ascending."""
    on = d.has[field] & mask
    cols, vals = d.cols[on], d.vals[field][on]
    order = np.lexsort((cols, ~vals if desc else vals))   # ~v = -v - 1: descending without overflow
    return cols[order], vals[order]


def window(pair, offset=0, limit=None):
    cols, vals = pair
    hi = None if limit is None else offset + limit
    return cols[offset:hi], vals[offset:hi]


def call_text(field, filt="", limit=None, offset=None, desc=None):
    args = ([filt] if filt else []) + [f"field={field}"]
    if limit is not None:
        args.append(f"limit={limit}")
    if offset is not None:
        args.append(f"offset={offset}")
    if desc is not None:
        args.append(f"sort-desc={'true' if desc else 'false'}")
    return "Sort(" + ", ".join(args) + ")"


def check(got, want, what=""):
    """``got`` (a SortedColumns) holds exactly the oracle's pair ``want``."""
    assert got.columns.dtype == np.uint64 and got.values.dtype == np.int64, what
    assert got.columns.tolist() == want[0].tolist(), what
    assert got.values.tolist() == want[1].tolist(), what


def tie_group(vals, value=None):
    """[lo, hi) of the positions holding ``value`` in the ordered ``vals``
    (None: the value held most often)."""
    if not len(vals):
        return 0, 0
    if value is None or not (vals == value).any():
        u, c = np.unique(vals, return_counts=True)
        value = u[np.argmax(c)]
    at = np.flatnonzero(vals == value)
    return int(at[0]), int(at[-1]) + 1


def cut_limits(vals, value=None):
    """Limits that put the cut before, inside (first, a middle and the last
    member) and after the tie group of ``value``, and 0, 1, N - 1, N, N + 1."""
    n = len(vals)
    lo, hi = tie_group(vals, value)
    out = {0, 1, n - 1, n, n + 1, lo, lo + 1, (lo + hi) // 2, hi - 1, hi, hi + 1}
    return sorted(x for x in out if x >= 0)
