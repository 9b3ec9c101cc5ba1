"""Fixture and numpy oracle of the set-like Extract() tests on the device
(tests/test_gpu_extract_rows.py): tests/topk_util.py's ``Data`` -- three shards
with a gap, keys 0, 7 and 15, 70 rows in field a in all three encodings,
lane-owned and cooperative arrays, a row at one key only, ghost columns, row
ids above 2^40 -- and, added by subclassing: a mutex field mx, a bool field b,
a time field t and a keyed set field ks.  Every expected value is exact; the
fixture is never changed after it is built."""
import datetime as dt

import numpy as np

from tests.helpers import SW
from tests.topk_util import A_IDS, BIG_ROW, SHARDS, U, Data

MX_IDS = (0, 2, 3, 77, BIG_ROW + 1)      # rows of the mutex field
T_IDS = (2, 11, 1 << 41)                 # rows of the time field
KS_KEYS = ("ab", "cd", "zz")
GHOST = f"Row(a={A_IDS[4]})"             # the ghost columns: they hold exactly that row of a
ONE = "Row(f=6)"                         # one column, in the last shard
FILTERS = ["Row(f=1)", "Intersect(Row(f=1), Row(g=1))", "Not(Row(f=1))", "Row(w > 500)", "Row(f=9)", ONE, GHOST]


class RowsData(Data):
    """``Data`` plus: f=6, one column of the key-7 stretch of the last shard
    (row A_IDS[1] of a, a run, covers it); mx, a mutex with the five rows
    MX_IDS over 60 % of all columns, ghost columns included -- every column in
    at most one row; b, a bool over 40 %; t, a time field (quantum YMD, bits
    imported with timestamps) with the rows T_IDS; ks, a keyed set field on
    the first nine columns of Row(f=1)."""

    def __init__(self, n=10000, seed=53):
        super().__init__(n, seed)
        rng = np.random.default_rng(seed + 1)
        N = len(self.cols)
        off = self.cols % np.uint64(SW)
        in_last = (self.cols // np.uint64(SW)) == np.uint64(SHARDS[-1])
        one = np.zeros(N, bool)
        one[np.flatnonzero(in_last & self.rows["a"][A_IDS[1]])[17]] = True
        self.rows["f"][6] = one
        self.one_col = int(self.cols[one][0])
        assert SW != 1 << 20 or (off[one][0] >> np.uint64(16)) == 7
        self.mx_has = rng.random(N) < 0.6
        self.mx_row = np.asarray(MX_IDS, np.uint64)[rng.integers(0, len(MX_IDS), N)]
        self.b_has = rng.random(N) < 0.4
        self.b_val = rng.random(N) < 0.5
        self.more = {
            "mx": {r: self.mx_has & (self.mx_row == np.uint64(r)) for r in MX_IDS},
            "b": {0: self.b_has & ~self.b_val, 1: self.b_has & self.b_val},
            "t": {r: rng.random(N) < p for r, p in zip(T_IDS, (0.3, 0.05, 0.01))},
        }
        f1 = np.flatnonzero(self.rows["f"][1])[:9]
        self.ks = {int(self.cols[p]): sorted({KS_KEYS[k % 2]} | ({"zz"} if k == 0 else set()))
                   for k, p in enumerate(f1.tolist())}

    def mask(self, filt):
        if filt == ONE:
            return self.rows["f"][6]
        if filt == GHOST:
            return self.rows["a"][A_IDS[4]]
        return super().mask(filt)

    def load(self, env):
        super().load(env)
        env.field("i", "mx", type="mutex")
        env.field("i", "b", type="bool")
        env.field("i", "t", type="time", time_quantum="YMD")
        env.field("i", "ks", keys=True)
        idx = env.holder.index("i")
        for fname, rows in self.more.items():
            for r, m in rows.items():
                k = int(m.sum())
                ts = [dt.datetime(2019, 3, 1 + (r % 20))] * k if fname == "t" else None
                idx.field(fname).import_bits(np.full(k, r, np.uint64), self.cols[m], ts)
        env.q("i", " ".join(f'Set({c}, ks="{k}")' for c, keys in self.ks.items() for k in keys))

    def columns(self, filt):
        """The filter's columns, ascending."""
        return np.sort(self.cols[self.mask(filt)])

    def cells(self, field, columns):
        """The oracle's cell of ``field`` per column: the ascending rows of a
        set or time field; the row of a mutex or the value of a bool, or None."""
        order = np.argsort(self.cols)
        at = order[np.searchsorted(self.cols[order], columns)]
        assert (self.cols[at] == columns).all()
        if field == "mx":
            return [int(r) if ok else None for r, ok in zip(self.mx_row[at].tolist(), self.mx_has[at].tolist())]
        if field == "b":
            return [bool(v) if ok else None for v, ok in zip(self.b_val[at].tolist(), self.b_has[at].tolist())]
        if field == "ks":
            return [self.ks.get(int(c), []) for c in columns.tolist()]
        rows = self.rows[field] if field in self.rows else self.more[field]
        ids = sorted(rows)
        member = np.stack([rows[r][at] for r in ids], axis=1) if len(at) else np.zeros((0, len(ids)), bool)
        return [[ids[k] for k in np.flatnonzero(m).tolist()] for m in member]


def call_text(filt, fields, offset=None, limit=None):
    args = [filt] + [f"Rows(field={f})" for f in fields]
    if limit is not None:
        args.append(f"limit={limit}")
    if offset is not None:
        args.append(f"offset={offset}")
    return "Extract(" + ", ".join(args) + ")"


TYPES = {"a": "[]uint64", "n": "[]uint64", "t": "[]uint64", "mx": "uint64", "b": "bool", "w": "int64"}


def check(d, table, fields, columns):
    """``table`` holds exactly ``columns`` and the oracle's cells of the
    set-like ``fields`` (int fields are skipped), in well-formed vectors."""
    assert table.columns.dtype == np.uint64 and table.columns.tolist() == columns.tolist()
    assert table.fields == [(f, TYPES[f]) for f in fields]
    for i, f in enumerate(fields):
        a, b = table.data[i]
        if TYPES[f] == "int64":
            continue
        if TYPES[f] == "[]uint64":
            assert a.dtype == np.int64 and b.dtype == np.uint64 and len(a) == len(columns) + 1
            assert a[0] == 0 and a[-1] == len(b) and (np.diff(a) >= 0).all()
        else:
            assert b.dtype == bool and len(a) == len(b) == len(columns)
            assert a.dtype == (np.bool_ if f == "b" else np.uint64) and not a[~b].any(), "a null carries a value"
        assert table.cells(i) == d.cells(f, columns), f
