"""Fixture and numpy oracle shared by the GroupBy(..., aggregate=Sum(field=))
tests.  Every expected value is an exact integer computed from the generated
columns; the fixture is never changed after it is built."""
import itertools

import numpy as np

from tests.helpers import SW

SHARDS = (0, 1, 3)    # shard 2 is absent
U = SW // 16          # columns per sixteenth of a shard (one container key at 2^20)
A_ROWS = tuple(range(1, 10))
B_ROWS = tuple(range(5))
C_ROWS = tuple(range(3))
BIG_RUN = (1 << 38) + 5   # the value of the constant stretch in `big`


class Data:
    """Per shard: ``n`` consecutive columns with random values from key 0
    (bitmap planes from n > 8192), ``n`` consecutive columns holding one value
    from key 7 (run containers: exists row and planes), 300 scattered columns
    in key 15 (arrays) and one column that exists without a value anywhere.

    Int fields: v -2000 .. 2000 (depth 11, base 0); w 100 .. 1100 (base 100),
    missing on every 5th column; big depth 40, magnitudes up to 2^39.

    Group fields: a, 9 rows -- 1 a random half of everything (a dense bitmap),
    2 the whole constant stretch (a run), 3 scattered columns of the constant
    stretch only (nothing outside key 7), 4 only columns without a value in w,
    5 .. 9 sparse random columns (arrays); b, 5 rows, and c, 3 rows: every
    valued column in exactly one row of each.  Filter rows f=1 and g=1."""

    def __init__(self, n=10000, seed=31):
        rng = np.random.default_rng(seed)
        cols, v, w, big, stretch = [], [], [], [], []
        pool_v = np.unique(np.concatenate([[-2000, -1, 0, 1, 2000], rng.integers(-2000, 2001, 35)]))
        pool_w = np.unique(rng.integers(100, 1101, 40))
        for s in SHARDS:
            a = s * SW + 100 + np.arange(n)
            b = s * SW + 7 * U + 50 + np.arange(n)
            c = s * SW + 15 * U + np.sort(rng.choice(min(U - 1, 40000), 300, replace=False))
            e = np.array([s * SW + 3 * U + 7])
            cols += [a, b, c, e]
            stretch += [np.zeros(n, int), np.ones(n, int), np.full(300, 2), np.full(1, 3)]
            v += [rng.choice(pool_v, n), np.full(n, -37), rng.choice(pool_v, 300), [0]]
            w += [rng.choice(pool_w, n), np.full(n, 612), rng.choice(pool_w, 300), [0]]
            big += [rng.integers(-(1 << 20), 1 << 20, n), np.full(n, BIG_RUN),
                    np.concatenate([[-(1 << 39), 1 << 39], rng.integers(-(1 << 39) + 1, 1 << 39, 298)]), [0]]
        self.cols = np.concatenate(cols).astype(np.uint64)
        assert len(np.unique(self.cols)) == len(self.cols)
        N = len(self.cols)
        st = np.concatenate(stretch)
        valued = st != 3
        self.vals = {"v": np.concatenate(v).astype(np.int64), "w": np.concatenate(w).astype(np.int64),
                     "big": np.concatenate(big).astype(np.int64)}
        self.has = {"v": valued, "big": valued, "w": valued & (np.arange(N) % 5 != 0)}
        arow = {1: rng.random(N) < 0.5, 2: st == 1, 3: (st == 1) & (np.arange(N) % 97 == 0),
                4: ~self.has["w"] & (rng.random(N) < 0.3)}
        for r in range(5, 10):
            arow[r] = valued & (rng.random(N) < 0.02)
        bsel, csel = rng.integers(0, 5, N), rng.integers(0, 3, N)
        self.rows = {"a": arow, "b": {r: valued & (bsel == r) for r in B_ROWS},
                     "c": {r: valued & (csel == r) for r in C_ROWS},
                     "f": {1: rng.random(N) < 0.5}, "g": {1: rng.random(N) < 0.3}}
        assert arow[4].any() and not (arow[4] & self.has["w"]).any()

    def mask(self, filt):
        f1, g1 = self.rows["f"][1], self.rows["g"][1]
        return {"": np.ones(len(self.cols), bool), "Row(f=1)": f1, "Intersect(Row(f=1), Row(g=1))": f1 & g1,
                "Not(Row(f=1))": ~f1, "Row(w > 500)": self.has["w"] & (self.vals["w"] > 500)}[filt]

    def load(self, env):
        env.create_index("i", track_existence=True)
        for name in ("a", "b", "c", "f", "g"):
            env.field("i", name)
        env.field("i", "v", type="int", min=-2000, max=2000)
        env.field("i", "w", type="int", min=100, max=1100, base=100)
        env.field("i", "big", type="int", min=-(1 << 39), max=1 << 39)
        idx = env.holder.index("i")
        for name in ("v", "w", "big"):
            idx.field(name).import_values(self.cols[self.has[name]], self.vals[name][self.has[name]])
        for fname, rows in self.rows.items():
            for r, m in rows.items():
                idx.field(fname).import_bits(np.full(int(m.sum()), r, np.uint64), self.cols[m])
        idx.existence_field().import_bits(np.zeros(len(self.cols), np.uint64), self.cols)

    def expected(self, fields, vfield, filt="", limit=None, previous=None, offset=None, keep=None, shards=None):
        """[(key, count, sum, sum_count)] of GroupBy(Rows(f) for f in fields,
        filter=filt, aggregate=Sum(field=vfield)) in result order; ``keep``
        restricts the rows of a field ({field: rows}), vfield None = no
        aggregate (sum members None)."""
        base = self.mask(filt)
        if shards is not None:
            base = base & np.isin(self.cols // np.uint64(SW), np.asarray(shards, np.uint64))
        out = []
        rows = [[r for r in sorted(self.rows[f]) if keep is None or f not in keep or r in keep[f]] for f in fields]
        for key in itertools.product(*rows):
            m = base
            for f, r in zip(fields, key):
                m = m & self.rows[f][r]
            if not m.any():
                continue
            if previous is not None and key <= tuple(previous):
                continue
            if vfield is None:
                out.append((key, int(m.sum()), None, None))
            else:
                hm = m & self.has[vfield]
                out.append((key, int(m.sum()), int(self.vals[vfield][hm].sum()), int(hm.sum())))
        if limit is not None:
            out = out[:limit]
        if offset is not None:
            out = out[offset:]
        return out


def call_text(fields, vfield=None, filt="", limit=None, previous=None, offset=None, children=None):
    parts = list(children) if children is not None else [f"Rows({f})" for f in fields]
    if filt:
        parts.append(f"filter={filt}")
    if limit is not None:
        parts.append(f"limit={limit}")
    if previous is not None:
        parts.append("previous=[" + ", ".join(str(p) for p in previous) + "]")
    if offset is not None:
        parts.append(f"offset={offset}")
    if vfield is not None:
        parts.append(f"aggregate=Sum(field={vfield})")
    return "GroupBy(" + ", ".join(parts) + ")"


def flat(groups):
    """list[GroupCount] -> [(key, count, sum, sum_count)]."""
    return [(g.key(), g.count, g.sum, g.sum_count) for g in groups]
