"""Shared pieces of the Distinct() tests: the numpy oracle (np.unique split by
sign), the call text, the filter list and the loader run on the host
(tests/test_distinct.py) and on the device (tests/test_gpu_distinct.py).

A fixture ``d`` has ``cols`` (uint64, every column that holds a value
somewhere), ``vals`` {int field: int64 per column}, ``has`` {int field: mask of
the columns holding a value in it}, ``rows`` {row of set field f: mask},
``extra`` (columns that exist and hold no value; they sit in row 1 of f) and
``schema`` {int field: FieldOptions keywords}."""
from __future__ import annotations

import numpy as np


def oracle(values):
    """(sorted distinct values >= 0, sorted |v| of the distinct values < 0)."""
    u = np.unique(np.asarray(values, dtype=np.int64))
    return u[u >= 0].tolist(), sorted((-u[u < 0]).tolist())


def flat(r):
    """A SignedRow as the oracle's pair of lists."""
    return [int(x) for x in r.pos.columns()], [int(x) for x in r.neg.columns()]


def call_text(field: str, filt: str = "") -> str:
    return f"Distinct({filt + ', ' if filt else ''}field={field})"


# none, a plain row, an intersection, a negation, a BSI predicate on another
# field (``other``), all-negative and all-non-negative (by v), one column, a
# row that does not exist, two rows that exist and share no column
def filters(d, other="w", bound=500):
    """[(filter text, mask over d.cols)]."""
    r = d.rows
    return [
        ("", np.ones(len(d.cols), bool)),
        ("Row(f=1)", r[1]),
        ("Intersect(Row(f=1), Row(f=4))", r[1] & r[4]),
        ("Not(Row(f=1))", ~r[1]),
        (f"Row({other} > {bound})", d.has[other] & (d.vals[other] > bound)),
        ("Row(f=2)", r[2]),
        ("Row(f=3)", r[3]),
        ("Row(f=5)", r[5]),
        ("Row(f=9)", np.zeros(len(d.cols), bool)),
        ("Intersect(Row(f=2), Row(f=3))", r[2] & r[3]),
    ]


def standard_rows(d, rng):
    """Rows of f over a fixture with int field v: 1 a random half, 4 a random
    third, 2 / 3 the columns whose v is negative / non-negative, 5 exactly one
    column."""
    n = len(d.cols)
    v = d.vals["v"]
    return {1: rng.random(n) < 0.5, 4: rng.random(n) < 0.33, 2: d.has["v"] & (v < 0), 3: d.has["v"] & (v >= 0),
            5: np.arange(n) == n // 2}


def considered(d, field, mask):
    return d.vals[field][d.has[field] & mask]


def load(env, d, index="i"):
    env.create_index(index, track_existence=True)
    env.field(index, "f")
    idx = env.holder.index(index)
    for name, opts in d.schema.items():
        env.field(index, name, type="int", **opts)
        idx.field(name).import_values(d.cols[d.has[name]], d.vals[name][d.has[name]])
    for row, m in d.rows.items():
        c = np.concatenate([d.cols[m], d.extra]) if row == 1 else d.cols[m]
        if len(c):
            idx.field("f").import_bits(np.full(len(c), row, np.uint64), c)
    every = np.concatenate([d.cols, d.extra])
    idx.existence_field().import_bits(np.zeros(len(every), np.uint64), every)
