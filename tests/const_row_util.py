"""Shared pieces of the ConstRow() and Extract(Sort()) tests, run on the host
(tests/test_const_row.py, tests/test_extract_sort.py) and on the device
(tests/test_gpu_const_row.py, tests/test_gpu_extract_sort.py): the call text,
the numpy oracles of the row and of the dense device view, random trees with
ConstRow leaves, and the gather behind Extract(Sort())."""
from __future__ import annotations

import numpy as np

from tests.helpers import SW


def text(cols) -> str:
    """ConstRow(columns=[...]) of the columns as given (order and duplicates kept)."""
    return "ConstRow(columns=[" + ",".join(str(int(c)) for c in cols) + "])"


def row_of(cols, shards) -> list:
    """The oracle's row: the distinct listed columns that lie in ``shards``, ascending."""
    u = np.unique(np.asarray(list(cols), dtype=np.uint64))
    return u[np.isin(u // np.uint64(SW), np.asarray(list(shards), dtype=np.uint64))].tolist()


def view_oracle(cols, dshards, arena_width):
    """(words uint32[S * 16, 2048], cards int64[S * 16]) of the dense view the
    device writes for ``cols`` over the device shards ``dshards``."""
    S = len(dshards)
    words = np.zeros((S * 16, 2048), np.uint32)
    for c in np.unique(np.asarray(list(cols), dtype=np.uint64)).tolist():
        ds, x = divmod(c, arena_width)
        if ds in dshards:
            u = dshards.index(ds) * 16 + (x >> 16)
            words[u, (x & 0xffff) >> 5] |= np.uint32(1 << (x & 31))
    cards = np.array([sum(bin(int(w)).count("1") for w in row[row != 0]) for row in words], np.int64)
    return words, cards


def meta_oracle(cards):
    """The meta words of a dense one-row view: key | bitmap << 4 | card << 6 | (u * 512) << 23."""
    u = np.arange(len(cards), dtype=np.int64)
    return (u & 15) | (2 << 4) | (cards << 6) | ((u * 512) << 23)


def random_tree(rng, lists, rows, depth=3) -> str:
    """A random bitmap call over ConstRow leaves (``lists``: column lists) and
    plain rows (``rows``: call texts), at most ``depth`` operators deep."""
    if depth == 0 or rng.random() < 0.25:
        if rng.random() < 0.6:
            return text(lists[int(rng.integers(len(lists)))])
        return rows[int(rng.integers(len(rows)))]
    op = ["Intersect", "Union", "Difference", "Xor", "Not", "Shift"][int(rng.integers(6))]
    if op == "Not":
        return f"Not({random_tree(rng, lists, rows, depth - 1)})"
    if op == "Shift":
        return f"Shift({random_tree(rng, lists, rows, depth - 1)}, n={int(rng.integers(0, 70))})"
    kids = [random_tree(rng, lists, rows, depth - 1) for _ in range(int(rng.integers(2, 4)))]
    return f"{op}({', '.join(kids)})"


def extract_sort_text(sort_text, fields, offset=None, limit=None) -> str:
    args = [sort_text] + [f"Rows(field={f})" for f in fields]
    if limit is not None:
        args.append(f"limit={limit}")
    if offset is not None:
        args.append(f"offset={offset}")
    return "Extract(" + ", ".join(args) + ")"


def cut(seq, offset=0, limit=None):
    return seq[offset:] if limit is None else seq[offset:offset + limit]
