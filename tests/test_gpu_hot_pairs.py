"""Hot-pair table (DeviceView.ensure_hot, pair_kernels.hip pair_build): the
per-shard intersection counts of a view's hottest rows with each other,
looked up instead of counted.  Every count is compared exactly with the host
roaring oracle, with the table and without it."""
import numpy as np
import pytest

from pilosa_amd import _roaring as R

pytestmark = pytest.mark.gpu

S, NKEYS, H = 3, 2, 8
WIDTH = 1 << 20
EDGE = np.array([0, 31, 32, 65535], np.int64)
T = 2048   # DeviceView.TWIN_CUTOFF's default: arrays above it are read through twins at 64 queries per wave
# the 8 rows with the most bits; container size per (shard, key), None = absent
HOT = {
    1: [[1500, 1500]] * 3,                       # array below the twin cutoff
    2: [[3000, 3000]] * 3,                       # array above it
    3: [[4096, 4096]] * 3,                       # largest array
    4: [[4097, 4097]] * 3,                       # smallest bitmap
    5: [[30000, 30000]] * 3,                     # bitmap
    6: [["run", 4000], [4000, "run"], ["run", "run"]],
    7: [[2500, 2500], [None, None], [2500, 2500]],   # absent from shard 1
    8: [[2600, None]] * 3,                       # absent from key 1
}
NEW_ROW = 0         # below every row: adding it shifts every dense index
COLD_N = (1, 8, 9, 64, 65, 511, 512, 513, 1000, 700, 300, 100, 40, 4)
COLD = {10 + i: [[n, n]] * 3 for i, n in enumerate(COLD_N)}
COLD[24] = [[5000, None], [None, None], [None, None]]      # a cold bitmap
COLD[25] = [[None, "srun"], [None, None], [None, "srun"]]  # a cold run
EMPTY = 99          # no such row: dense index -1
HOT_ROWS, COLD_ROWS = sorted(HOT), sorted(COLD)


def _vals(rng, n):
    if n == "run":
        return np.concatenate([np.arange(0, 40000), [65535]])
    if n == "srun":
        return np.arange(0, 3001)
    if n <= 4:
        return EDGE[:n].copy()
    return np.sort(np.concatenate([EDGE, rng.choice(np.arange(33, 65535), n - 4, replace=False)]))


def _build(seed, spec):
    """Per-shard fragments of ``spec``; only the run containers are optimised
    (a 4096-value container stays an array)."""
    rng = np.random.default_rng(seed)
    frags = []
    for s in range(S):
        pos, runs = [], []
        for row, per_shard in spec.items():
            for j, n in enumerate(per_shard[s]):
                if n is None:
                    continue
                v = _vals(rng, n)
                (runs if isinstance(n, str) else pos).append(
                    (np.uint64(row) * np.uint64(16) + np.uint64(j)) * np.uint64(65536) + v.astype(np.uint64))
        b = R.Bitmap(np.concatenate(pos))
        if runs:
            rb = R.Bitmap(np.concatenate(runs))
            rb.optimize()
            b = b.union(rb)
        frags.append(b)
    return frags


class Oracle:
    """Per-shard intersection counts from the host fragments (rows cached)."""

    def __init__(self):
        self.rows = {}

    def row(self, frags, s, r):
        k = (id(frags), s, r)
        if k not in self.rows:
            self.rows[k] = frags[s].offset_range(0, r * WIDTH, (r + 1) * WIDTH)
        return self.rows[k]

    def forget(self, frags, s):
        for k in [k for k in self.rows if k[0] == id(frags) and k[1] == s]:
            del self.rows[k]

    def per_shard(self, prs):
        """prs = [(frags a, row a, frags b, row b)] -> int64[Q, S]."""
        return np.array([[self.row(fa, s, a).intersection_count(self.row(fb, s, b)) for s in range(S)]
                         for fa, a, fb, b in prs], np.int64)


def _make(dev, patchable=False):
    from pilosa_amd.ops.device import DeviceView

    frags = _build(41, {**HOT, **COLD})
    view = DeviceView.from_bitmaps(frags, dev, shards=list(range(S)), patchable=patchable)
    view.HOTPAIR_ROWS = H
    view.HOTPAIR_MIN_CONTAINERS = 0
    return frags, view


@pytest.fixture(scope="module")
def world():
    """One read-only view with its table, a second view over the same shards
    (its own table) and the oracle shared by the read-only tests."""
    import torch

    dev = torch.device("cuda:0")
    frags, view = _make(dev)
    kinds = {t for f in frags for _, t, _ in f.container_info()}
    assert kinds == {"array", "bitmap", "run"}
    frags2 = _build(42, {1: HOT[1], 5: HOT[5], 12: COLD[12]})
    from pilosa_amd.ops.device import DeviceView
    view2 = DeviceView.from_bitmaps(frags2, dev, shards=list(range(S)))
    view2.HOTPAIR_ROWS = H
    view2.HOTPAIR_MIN_CONTAINERS = 0
    return dev, frags, view, frags2, view2, Oracle()


def _hot_ids(view):
    return [int(view.rows[d]) for d in view._hot.rows.tolist()]


def _check_table(view, frags, oracle, shards=range(S)):
    hp = view._hot
    ids = _hot_ids(view)
    got = hp.counts.cpu().numpy()
    assert got.shape == (S, hp.h, hp.h)
    for s in shards:
        for i, a in enumerate(ids):
            for j, b in enumerate(ids):
                want = oracle.row(frags, s, a).intersection_count(oracle.row(frags, s, b))
                assert got[s, i, j] == want, (s, a, b)


def test_table_matches_host(world):
    dev, frags, view, _, _, oracle = world
    assert view.ensure_hot() and view.hot_fresh()
    assert view.hot_stats["full_builds"] == 1
    assert _hot_ids(view) == HOT_ROWS and view._hot.h == H
    slot = view._hot.slot.cpu().numpy()
    assert sorted(slot[slot >= 0].tolist()) == list(range(H)) and (slot >= 0).sum() == H
    assert view._hot.valid.cpu().numpy().tolist() == [1] * S
    # H = 8 is one tile: every entry is filled, the diagonal holds the row counts
    _check_table(view, frags, oracle)
    rec = view.viewdev()
    assert int(rec["hot_counts"]) != 0 and int(rec["hot_h"]) == H
    assert int(view.viewdev(hot=False)["hot_counts"]) == 0
    assert view.nbytes() >= S * H * H * 4


def _batch(world, n):
    """n queries cycling over every kind of pair; (exprs, oracle pairs, how
    many of them both views' tables answer)."""
    from pilosa_amd.ops.device import Leaf, Op

    dev, frags, view, frags2, view2, _ = world
    base = []
    for a in HOT_ROWS:                 # hot x hot, both orders over the batch, and a == a
        for b in HOT_ROWS:
            if (a + b) % 3 != 1 or a == b:
                base.append((view, frags, a, view, frags, b))
    for k, c in enumerate(COLD_ROWS):  # hot x cold, cold x hot
        base.append((view, frags, HOT_ROWS[k % H], view, frags, c))
        base.append((view, frags, c, view, frags, HOT_ROWS[(k + 3) % H]))
    for k, c in enumerate(COLD_ROWS):  # cold x cold, cold a == a
        base.append((view, frags, c, view, frags, COLD_ROWS[(k + 5) % len(COLD_ROWS)]))
    base.append((view, frags, 13, view, frags, 13))
    base += [(view, frags, 5, view, frags, EMPTY), (view, frags, EMPTY, view, frags, 2),
             (view, frags, EMPTY, view, frags, 17)]
    # two pairs across the two views (hot rows of both: no table spans views), one inside the second
    base += [(view, frags, 5, view2, frags2, 5), (view2, frags2, 1, view, frags, 3), (view2, frags2, 1, view2, frags2, 5)]
    rng = np.random.default_rng(n)
    order = rng.permutation(len(base))
    # the five kinds lead every batch, however short
    lead = [base[0], base[-1], base[-3], base[-5], [b for b in base if b[2] in COLD and b[5] in COLD][0]]
    items = (lead + [base[i] for i in order] * (n // len(base) + 1))[:n]
    exprs = [Op("and", (Leaf(va, a), Leaf(vb, b))) for va, _, a, vb, _, b in items]
    prs = [(fa, a, fb, b) for _, fa, a, _, fb, b in items]
    hot2 = set(_hot_ids(view2)) if getattr(view2, "_hot", None) is not None else set()
    tabled = sum(1 for va, _, a, vb, _, b in items
                 if va is vb and ((va is view and a in HOT and b in HOT) or (va is view2 and a in hot2 and b in hot2)))
    return exprs, prs, tabled


def _marked(eng, handle):
    """Entries of the pairs buffer that pair_build answered from a table."""
    import torch
    Q, S_, tv, parts = handle[:4]
    (tp, ti, kind, n), = parts
    pairs = torch.empty(S_ * 16 * n * 2, dtype=torch.int32, device=eng.device)
    partial = torch.empty(S_ * 16 * n, dtype=torch.int32, device=eng.device)
    eng.ext.and2_count(tp, tv, S_, pairs, partial, eng.and2_cq, 6)
    x = pairs.view(S_, 16, n, 2)[..., 0].cpu().numpy()
    assert (x[:, 1:] != -2).all()     # the marker rides in key 0's entry only
    return x[:, 0] == -2              # [S, n]


# 5 / 40 / 100: serving variant 39 at 4 / 32 / 16 queries per wave; 200: v6 at 32; 2100: 64 per wave (twins: 63)
@pytest.mark.parametrize("n", [5, 40, 100, 200, 2100])
def test_batches_match_host_with_and_without_table(world, n, monkeypatch):
    from pilosa_amd.ops.device import GpuEngine

    dev, frags, view, frags2, view2, oracle = world
    assert view.ensure_hot() and view2.ensure_hot()
    exprs, prs, tabled = _batch(world, n)
    assert 0 < tabled < n
    want = oracle.per_shard(prs)
    eng = GpuEngine(dev)
    assert eng.use_hot
    handle = eng.prepare_count(exprs)
    assert view.hot_fresh() and view2.hot_fresh()
    if n > 2048:
        assert view.twin_fresh() and handle[4] == 2
    assert int(_marked(eng, handle).sum()) == tabled * S
    got = eng.to_host(eng.launch_count(handle)).numpy()
    np.testing.assert_array_equal(got, want.sum(axis=1))
    np.testing.assert_array_equal(eng.count_per_shard(exprs), want)
    # the same batch without the table
    monkeypatch.setenv("PILOSA_HOTPAIR", "0")
    plain = GpuEngine(dev)
    assert not plain.use_hot
    handle = plain.prepare_count(exprs)
    assert int(_marked(plain, handle).sum()) == 0
    np.testing.assert_array_equal(plain.to_host(plain.launch_count(handle)).numpy(), got)
    np.testing.assert_array_equal(plain.count_per_shard(exprs), want)


def _write(view, frags, oracle, si, row, key, lo, hi, n):
    """Set n new values in [lo, hi) of (row, key) of shard si on the device and in the host fragment."""
    base = row * WIDTH + key * 65536
    pos = np.array([base + v for v in range(lo, hi) if not frags[si].contains(base + v)][:n], np.uint64)
    assert len(pos) == n
    assert view.apply_positions(si, pos, clear=False)
    frags[si].add_many(pos, True)
    oracle.forget(frags, si)


def test_write_to_hot_row_never_reads_a_stale_slice():
    import torch
    from pilosa_amd.ops.device import GpuEngine, Leaf, Op

    dev = torch.device("cuda:0")
    frags, view = _make(dev, patchable=True)
    oracle = Oracle()
    pairs = [(a, b) for a in HOT_ROWS for b in HOT_ROWS if a <= b] + [(2, 12), (15, 5), (12, 15)]
    exprs = [Op("and", (Leaf(view, a), Leaf(view, b))) for a, b in pairs]
    prs = lambda: [(frags, a, frags, b) for a, b in pairs]   # noqa: E731
    nhot = sum(1 for a, b in pairs if a in HOT and b in HOT)
    eng = GpuEngine(dev)
    np.testing.assert_array_equal(eng.count_per_shard(exprs), oracle.per_shard(prs()))
    assert view.hot_fresh() and view.hot_stats == {"full_builds": 1, "invalidated_shards": 0, "refreshed_shards": 0}

    # 1. a write into hot row 2 of shard 1.  By default no slice is recomputed
    # inside the request that finds it written (one costs as much as several
    # serving-size batches): it is masked out, the other shards keep the table
    assert view.HOTPAIR_REFRESH_SHARDS == 0
    before = view._hot.counts[1].cpu().numpy().copy()
    _write(view, frags, oracle, 1, 2, 1, 40000, 50000, 60)
    assert not view.hot_fresh() and int(view.viewdev()["hot_counts"]) == 0   # not passed until synchronised
    want = oracle.per_shard(prs())
    handle = eng.prepare_count(exprs)
    assert view.hot_fresh()
    assert view.hot_stats == {"full_builds": 1, "invalidated_shards": 1, "refreshed_shards": 0}
    assert view._hot.valid.cpu().numpy().tolist() == [1, 0, 1] and view._hot.pending.tolist() == [False, True, False]
    marked = _marked(eng, handle)
    assert marked[1].sum() == 0 and marked[0].sum() == nhot and marked[2].sum() == nhot
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want.sum(axis=1))
    np.testing.assert_array_equal(eng.count_per_shard(exprs), want)
    # the masked slice is indeed stale: reading it would have been wrong
    ids = _hot_ids(view)
    i2 = ids.index(2)
    assert before[i2, i2] + 60 == oracle.row(frags, 1, 2).count()
    np.testing.assert_array_equal(view._hot.counts[1].cpu().numpy(), before)

    # 2. once the interval has passed the slice is recomputed, alone
    view.HOTPAIR_MIN_INTERVAL_S = 0.0
    handle = eng.prepare_count(exprs)
    assert view.hot_stats == {"full_builds": 1, "invalidated_shards": 1, "refreshed_shards": 1}
    assert view._hot.valid.cpu().numpy().tolist() == [1, 1, 1] and not view._hot.pending.any()
    _check_table(view, frags, oracle)
    assert int(_marked(eng, handle).sum()) == nhot * S
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want.sum(axis=1))

    # 3. with a refresh budget a written shard is recomputed before the next batch
    view.HOTPAIR_MIN_INTERVAL_S = 30.0
    view.HOTPAIR_REFRESH_SHARDS = 64
    _write(view, frags, oracle, 2, 5, 0, 0, 2000, 100)
    want = oracle.per_shard(prs())
    np.testing.assert_array_equal(eng.count_per_shard(exprs), want)
    assert view.hot_fresh()
    assert view.hot_stats == {"full_builds": 1, "invalidated_shards": 2, "refreshed_shards": 2}
    assert view._hot.valid.cpu().numpy().tolist() == [1, 1, 1]
    _check_table(view, frags, oracle)
    np.testing.assert_array_equal(eng.count(exprs), want.sum(axis=1))

    # 4. more runs of written shards than HOTPAIR_FULL_RUNS: every shard is recomputed at the interval
    view.HOTPAIR_REFRESH_SHARDS = 0
    view.HOTPAIR_FULL_RUNS = 0
    _write(view, frags, oracle, 0, 3, 1, 100, 300, 10)     # the 4096-value array becomes a bitmap
    want = oracle.per_shard(prs())
    np.testing.assert_array_equal(eng.count_per_shard(exprs), want)
    assert view._hot.valid.cpu().numpy().tolist() == [0, 1, 1]
    view.HOTPAIR_MIN_INTERVAL_S = 0.0
    np.testing.assert_array_equal(eng.count_per_shard(exprs), want)
    assert view.hot_stats == {"full_builds": 1, "invalidated_shards": 3, "refreshed_shards": 2 + S}
    assert view._hot.valid.cpu().numpy().tolist() == [1, 1, 1] and not view._hot.pending.any()
    _check_table(view, frags, oracle)


def test_new_row_drops_the_table_until_it_is_rebuilt():
    import torch
    from pilosa_amd.ops.device import GpuEngine, Leaf, Op

    dev = torch.device("cuda:0")
    frags, view = _make(dev, patchable=True)
    oracle = Oracle()
    pairs = [(a, b) for a in HOT_ROWS for b in HOT_ROWS if a < b] + [(2, 12), (12, 15), (6, 6)]
    eng = GpuEngine(dev)
    exprs = [Op("and", (Leaf(view, a), Leaf(view, b))) for a, b in pairs]
    np.testing.assert_array_equal(eng.count(exprs), oracle.per_shard([(frags, a, frags, b) for a, b in pairs]).sum(axis=1))
    assert view.hot_fresh()
    rows_gen = view.rows_gen
    # a new row below every other: every dense index shifts
    new = np.uint64(NEW_ROW) * np.uint64(WIDTH) + np.arange(100, 3100, dtype=np.uint64)
    assert view.apply_positions(0, new, clear=False)
    frags[0].add_many(new, True)
    oracle.forget(frags, 0)
    assert view.rows_gen == rows_gen + 1
    pairs += [(NEW_ROW, 2), (NEW_ROW, 12), (12, NEW_ROW), (NEW_ROW, NEW_ROW)]
    exprs = [Op("and", (Leaf(view, a), Leaf(view, b))) for a, b in pairs]
    want = oracle.per_shard([(frags, a, frags, b) for a, b in pairs])
    # inside the rebuild interval: no table is passed, answers are exact
    handle = eng.prepare_count(exprs)
    assert not view.hot_fresh() and int(view.viewdev()["hot_counts"]) == 0 and int(view.viewdev()["hot_slot"]) == 0
    assert int(_marked(eng, handle).sum()) == 0
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want.sum(axis=1))
    np.testing.assert_array_equal(eng.count_per_shard(exprs), want)
    # after it: rebuilt over the new directory
    view.HOTPAIR_MIN_INTERVAL_S = 0.0
    handle = eng.prepare_count(exprs)
    assert view.hot_fresh() and view.hot_stats["full_builds"] == 2
    assert _hot_ids(view) == HOT_ROWS     # the new row (3000 bits) is not among the 8 hottest
    _check_table(view, frags, oracle)
    assert int(_marked(eng, handle).sum()) > 0
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want.sum(axis=1))
    np.testing.assert_array_equal(eng.count_per_shard(exprs), want)


def test_small_views_carry_no_table_by_default():
    import torch
    from pilosa_amd.ops.device import DeviceView, GpuEngine, Leaf, Op

    dev = torch.device("cuda:0")
    frags = _build(41, {**HOT, **COLD})
    view = DeviceView.from_bitmaps(frags, dev, shards=list(range(S)))
    assert view.container_count < DeviceView.HOTPAIR_MIN_CONTAINERS
    eng = GpuEngine(dev)
    got = eng.count([Op("and", (Leaf(view, 5), Leaf(view, 6)))])
    assert getattr(view, "_hot", None) is None and not view.hot_fresh()
    assert got[0] == Oracle().per_shard([(frags, 5, frags, 6)]).sum()
