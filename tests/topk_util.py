"""Fixture and numpy oracle shared by the TopK(field=, k=) tests.  Every
expected value is an exact integer computed from the generated columns; the
fixture is never changed after it is built."""
import numpy as np

from tests.helpers import SW

SHARDS = (0, 1, 3)    # shard 2 is absent
U = SW // 16          # columns per sixteenth of a shard (one container key at 2^20)
BIG_ROW = (1 << 40) + 7
# 70 sparse row ids of the ranked field a: more than the 64 lanes of a wave
# streaming rows, and more than the four waves of a workgroup
A_IDS = tuple(i * i + 1 for i in range(69)) + (BIG_ROW,)
N_IDS = (0, 3, 4, 9, 100)          # rows of the cacheType none field
FILTERS = ["", "Row(f=1)", "Intersect(Row(f=1), Row(g=1))", "Not(Row(f=1))", "Row(w > 500)", "Row(f=9)"]
KS = [None, 0, 1, 5, 1000]         # absent, 0 (both: every row), 1, 5, more than the rows


class Data:
    """Per shard: ``n`` consecutive columns from key 0, ``n`` consecutive
    columns from key 7, 300 scattered columns in key 15 -- all of them in the
    existence field -- and 40 "ghost" columns in key 15 that exist nowhere but
    in row A_IDS[4] of a.

    Ranked field a (by position in A_IDS): 0 a random half of everything
    (bitmaps), 1 the whole key-7 stretch (a run), 2 scattered columns of the
    key-7 stretch only (one key), 3 sparse, absent from shard 1, 4 the ghost
    columns (it meets no filter), 5 = 6 and 7 = 8 the same columns (ties
    under every filter), 9 .. 68 random columns at densities from 0.05 % to
    20 % (arrays of a few values up to arrays of thousands), 69 (id > 2^40)
    sparse.  Field n (cacheType none): five rows.  Filter rows: f=1 a random
    half of keys 0 and 15 and the whole key-7 stretch (bitmap, run, array),
    g=1 a random 30 %; f=9 does not exist.  Int field w, 100 .. 1100, missing
    on every 5th column."""

    def __init__(self, n=10000, seed=53):
        rng = np.random.default_rng(seed)
        cols, stretch = [], []
        for s in SHARDS:
            pick = np.sort(rng.choice(min(U - 1, 40000), 340, replace=False))
            cols += [s * SW + 100 + np.arange(n), s * SW + 7 * U + 50 + np.arange(n),
                     s * SW + 15 * U + pick[:300], s * SW + 15 * U + pick[300:]]
            stretch += [np.zeros(n, int), np.ones(n, int), np.full(300, 2), np.full(40, 3)]
        self.cols = np.concatenate(cols).astype(np.uint64)
        assert len(np.unique(self.cols)) == len(self.cols)
        N = len(self.cols)
        st = np.concatenate(stretch)
        shard = (self.cols // np.uint64(SW)).astype(np.int64)
        self.exists = st != 3
        ex = self.exists
        self.has_w = ex & (np.arange(N) % 5 != 0)
        self.w = rng.integers(100, 1101, N)
        rows = {0: ex & (rng.random(N) < 0.5), 1: st == 1, 2: (st == 1) & (np.arange(N) % 97 == 0),
                3: ex & (shard != 1) & (rng.random(N) < 0.01), 4: st == 3}
        rows[5] = rows[6] = ex & (rng.random(N) < 0.03)
        rows[7] = rows[8] = ex & (rng.random(N) < 0.004)
        dens = np.geomspace(0.0005, 0.2, 60)
        for i in range(9, 69):
            rows[i] = ex & (rng.random(N) < dens[i - 9])
        rows[69] = ex & (rng.random(N) < 0.002)
        f1 = ex & ((st == 1) | (rng.random(N) < 0.5))
        self.rows = {"a": {A_IDS[i]: m for i, m in rows.items()},
                     "n": {r: ex & (rng.random(N) < p) for r, p in zip(N_IDS, (0.3, 0.01, 0.01, 0.2, 0.001))},
                     "f": {1: f1}, "g": {1: ex & (rng.random(N) < 0.3)}}
        assert all(m.any() for rr in self.rows.values() for m in rr.values())

    def mask(self, filt):
        f1, g1 = self.rows["f"][1], self.rows["g"][1]
        return {"": np.ones(len(self.cols), bool), "Row(f=1)": f1, "Intersect(Row(f=1), Row(g=1))": f1 & g1,
                "Not(Row(f=1))": self.exists & ~f1, "Row(w > 500)": self.has_w & (self.w > 500),
                "Row(f=9)": np.zeros(len(self.cols), bool)}[filt]

    def load(self, env):
        env.create_index("i", track_existence=True)
        for name in ("a", "f", "g"):
            env.field("i", name)
        env.field("i", "n", cache_type="none")
        env.field("i", "w", type="int", min=100, max=1100, base=100)
        idx = env.holder.index("i")
        idx.field("w").import_values(self.cols[self.has_w], self.w[self.has_w])
        for fname, rows in self.rows.items():
            for r, m in rows.items():
                idx.field(fname).import_bits(np.full(int(m.sum()), r, np.uint64), self.cols[m])
        idx.existence_field().import_bits(np.zeros(int(self.exists.sum()), np.uint64), self.cols[self.exists])

    def expected(self, field="a", filt="", k=None, shards=None):
        """[(row id, count)] of TopK(filt, field=field, k=k): the non-zero
        counts, count descending then id ascending, cut to k (None / 0: all)."""
        base = self.mask(filt)
        if shards is not None:
            base = base & np.isin(self.cols // np.uint64(SW), np.asarray(shards, np.uint64))
        out = [(r, int((m & base).sum())) for r, m in self.rows[field].items()]
        out = sorted((p for p in out if p[1] > 0), key=lambda p: (-p[1], p[0]))
        return out[:k] if k else out


def call_text(field="a", filt="", k=None):
    parts = ([filt] if filt else []) + [f"field={field}"] + ([f"k={k}"] if k is not None else [])
    return "TopK(" + ", ".join(parts) + ")"


def flat(pairs):
    """list[Pair] -> [(id, count)]."""
    return [(p.id, p.count) for p in pairs]
