"""Count(Intersect) with the table-answered queries compacted out of the pair
grid (pair_kernels.hip pair_split_kernel / hot_pair_sum_kernel and the pair
kernels that read the query count from device memory,
GpuEngine._and2_total).  Every answer is compared exactly with the host
roaring core and with the same batch on today's route
(PILOSA_PAIR_COMPACT=0); the split's two counters are read back from its
scratch to see which queries left the grid."""
import numpy as np
import pytest

from pilosa_amd import _roaring as R

pytestmark = pytest.mark.gpu

S, H = 3, 8
WIDTH = 1 << 20
# the 8 rows with the most bits; values per (shard, key), None = absent
HOT = {
    1: [[1500, 1500]] * 3,                       # array
    2: [[3000, 3000]] * 3,                       # array above the twin cutoff
    3: [[4096, 4096]] * 3,                       # largest array
    4: [[4097, 4097]] * 3,                       # smallest bitmap
    5: [[30000, 30000]] * 3,                     # bitmap
    6: [["run", 4000], [4000, "run"], ["run", "run"]],
    7: [[2500, 2500], [None, None], [2500, 2500]],   # absent from shard 1
    8: [[2600, None]] * 3,                       # absent from key 1
}
COLD_N = (1, 8, 9, 64, 65, 511, 512, 513, 1000, 700, 300, 100, 40, 4)
COLD = {10 + i: [[n, n]] * 3 for i, n in enumerate(COLD_N)}
COLD[24] = [[5000, None], [None, None], [None, None]]      # a cold bitmap
COLD[25] = [[None, "srun"], [None, None], [None, "srun"]]  # a cold run
EMPTY = 99          # no such row: dense index -1
HOT_ROWS, COLD_ROWS = sorted(HOT), sorted(COLD)
SPEC2 = {1: HOT[1], 5: HOT[5], 12: COLD[12]}    # the second view: every row has a slot


def _vals(rng, n):
    if n == "run":
        return np.concatenate([np.arange(0, 40000), [65535]])
    if n == "srun":
        return np.arange(0, 3001)
    edge = np.array([0, 31, 32, 65535], np.int64)
    if n <= 4:
        return edge[:n].copy()
    return np.sort(np.concatenate([edge, rng.choice(np.arange(33, 65535), n - 4, replace=False)]))


def _build(seed, spec):
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


class Host:
    """Count(Intersect) totals from the host fragments (rows cached)."""

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

    def totals(self, items):
        return np.array([sum(self.row(fa, s, a).intersection_count(self.row(fb, s, b)) for s in range(S))
                         for (_, fa), a, (_, fb), b in items], np.int64)


class Spy:
    """The kernel module with and2_count_total's {live, table-answered}
    counters read back after every call."""

    def __init__(self, ext):
        self._ext = ext
        self.counts = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def and2_count_total(self, *args):
        import torch
        self._ext.and2_count_total(*args)
        self.counts.append(tuple(args[7][:8].view(torch.int32).cpu().tolist()))


def _view(dev, frags, table=True, patchable=False):
    from pilosa_amd.ops.device import DeviceView

    view = DeviceView.from_bitmaps(frags, dev, shards=list(range(S)), patchable=patchable)
    if table:       # a view this small carries no table by default
        view.HOTPAIR_ROWS = H
        view.HOTPAIR_MIN_CONTAINERS = 0
    return view


def _engine(dev):
    from pilosa_amd.ops.device import GpuEngine

    eng = GpuEngine(dev)
    assert eng.use_hot and eng.use_compact
    eng.PAIR_COMPACT_MIN = 1
    eng.ext = Spy(eng.ext)
    return eng


@pytest.fixture(scope="module")
def world():
    import torch

    dev = torch.device("cuda:0")
    frags = _build(41, {**HOT, **COLD})
    frags2 = _build(42, SPEC2)
    v1, v2, v3 = _view(dev, frags), _view(dev, frags2), _view(dev, frags, table=False)
    return dev, (v1, frags), (v2, frags2), (v3, frags), Host()


def _hot_items(w, n):
    """n queries the first view's table answers (every unordered pair, a == a included, repeated)."""
    base = [(w, a, w, b) for a in HOT_ROWS for b in HOT_ROWS]
    return (base * (n // len(base) + 1))[:n]


def _live_items(w, w2, n):
    """n queries no table answers: hot x cold, cold x cold, an absent row, pairs across two views."""
    base = []
    for k, c in enumerate(COLD_ROWS):
        base.append((w, HOT_ROWS[k % H], w, c))
        base.append((w, c, w, HOT_ROWS[(k + 3) % H]))
        base.append((w, c, w, COLD_ROWS[(k + 5) % len(COLD_ROWS)]))
    base += [(w, 13, w, 13), (w, 5, w, EMPTY), (w, EMPTY, w, 2), (w, EMPTY, w, 17), (w, EMPTY, w, EMPTY)]
    base += [(w, 5, w2, 5), (w2, 1, w, 3), (w2, 12, w, 12)]
    return (base * (n // len(base) + 1))[:n]


def _mixed(w, w2, nhot, nlive, seed):
    """nhot table-answered queries (of both views) and nlive live ones, shuffled."""
    hot = _hot_items(w, nhot)
    for i, (a, b) in enumerate([(1, 5), (5, 1), (12, 12), (5, 12)]):   # the second view's own table
        if 3 * i + 1 < len(hot):
            hot[3 * i + 1] = (w2, a, w2, b)
    items = hot + _live_items(w, w2, nlive)
    order = np.random.default_rng(seed).permutation(len(items))
    return [items[i] for i in order]


def _exprs(items):
    from pilosa_amd.ops.device import Leaf, Op

    return [Op("and", (Leaf(va, a), Leaf(vb, b))) for (va, _), a, (vb, _), b in items]


def _check(dev, eng, items, host, monkeypatch, counts):
    """The batch on the compacted route (``counts`` = the {live,
    table-answered} pairs its launches must leave, [] = today's route), against
    the host and against the same batch under PILOSA_PAIR_COMPACT=0."""
    from pilosa_amd.ops.device import GpuEngine

    exprs = _exprs(items)
    want = host.totals(items)
    eng.ext.counts.clear()
    got = eng.to_host(eng.launch_count(eng.prepare_count(exprs))).numpy()
    print("counters", eng.ext.counts, "expected", counts)
    np.testing.assert_array_equal(got, want)
    assert eng.ext.counts == counts
    monkeypatch.setenv("PILOSA_PAIR_COMPACT", "0")
    plain = GpuEngine(dev)
    monkeypatch.delenv("PILOSA_PAIR_COMPACT")
    assert not plain.use_compact
    plain.PAIR_COMPACT_MIN = 1
    plain.ext = Spy(plain.ext)
    np.testing.assert_array_equal(plain.to_host(plain.launch_count(plain.prepare_count(exprs))).numpy(), got)
    assert plain.ext.counts == []
    return got


# 1 / 63 / 64 / 65: serving-size batches never take the route; 130: 32 queries per wave, 257: three tiles of 128
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 257])
def test_batch_sizes(world, n, monkeypatch):
    dev, w, w2, _, host = world
    nhot = (n * 3) // 5 if n > 1 else 1
    items = _mixed(w, w2, nhot, n - nhot, n)
    assert len(items) == n
    _check(dev, _engine(dev), items, host, monkeypatch, [(n - nhot, nhot)] if n > 128 else [])


def test_every_query_table_answered(world, monkeypatch):
    dev, w, w2, _, host = world
    items = _hot_items(w, 200)
    _check(dev, _engine(dev), items, host, monkeypatch, [(0, 200)])


def test_no_query_table_answered(world, monkeypatch):
    dev, w, w2, w3, host = world
    # a view without a table: the batch passes none, today's route
    items = [(w3, a, w3, b) for _, a, _, b in _hot_items(w, 100) + _live_items(w, w, 60)]
    eng = _engine(dev)
    _check(dev, eng, items, host, monkeypatch, [])
    assert getattr(w3[0], "_hot", None) is None
    # a table is passed and answers nothing: every query stays in the grid
    items = _live_items(w, w2, 150)
    _check(dev, eng, items, host, monkeypatch, [(150, 0)])
    # the table's view next to the view without one, hot rows of both
    items = _hot_items(w, 70) + [(w3, a, w3, b) for _, a, _, b in _hot_items(w, 70)] + [(w, 2, w3, 2), (w3, 5, w, 5)]
    _check(dev, eng, items, host, monkeypatch, [(72, 70)])


@pytest.mark.parametrize("nlive", [64, 65])
def test_live_queries_fill_one_wave_exactly_and_one_more(world, nlive, monkeypatch):
    dev, w, w2, _, host = world
    items = _mixed(w, w2, 100, nlive, nlive)
    _check(dev, _engine(dev), items, host, monkeypatch, [(nlive, 100)])


def test_two_views_2100_queries_at_64_per_wave(world, monkeypatch):
    """Above 2048 queries: 64 queries per wave with bitmap twins (variant 63),
    three tiles of the split, cross-view pairs live, same-view hot pairs
    answered by each view's own table."""
    dev, w, w2, _, host = world
    items = _mixed(w, w2, 1300, 800, 7)
    eng = _engine(dev)
    _check(dev, eng, items, host, monkeypatch, [(800, 1300)])
    assert w[0].twin_fresh()


def test_masked_shard_keeps_the_view_live_until_refreshed(monkeypatch):
    import torch

    dev = torch.device("cuda:0")
    frags = _build(41, {**HOT, **COLD})
    w = (_view(dev, frags, patchable=True), frags)
    view = w[0]
    host = Host()
    eng = _engine(dev)
    items = _mixed(w, w, 100, 60, 3)
    nhot = sum(1 for _, a, _, b in items if a in HOT and b in HOT)
    before = _check(dev, eng, items, host, monkeypatch, [(len(items) - nhot, nhot)])
    # a write into hot row 2 of shard 1: the slice is masked, not recomputed
    base = 2 * WIDTH + 65536
    pos = np.array([base + v for v in range(40000, 50000) if not frags[1].contains(base + v)][:60], np.uint64)
    assert view.apply_positions(1, pos, clear=False)
    frags[1].add_many(pos, True)
    host.forget(frags, 1)
    after = _check(dev, eng, items, host, monkeypatch, [(len(items), 0)])
    assert view._hot.valid.cpu().numpy().tolist() == [1, 0, 1]
    changed = np.array([2 in (a, b) for _, a, _, b in items])
    np.testing.assert_array_equal(after[~changed], before[~changed])
    assert (after[changed] >= before[changed]).all() and (after != before).any()
    # once the slice is recomputed the table answers again
    view.HOTPAIR_MIN_INTERVAL_S = 0.0
    again = _check(dev, eng, items, host, monkeypatch, [(len(items) - nhot, nhot)])
    assert view._hot.valid.cpu().numpy().tolist() == [1, 1, 1]
    np.testing.assert_array_equal(again, after)


def test_text_route_with_repeated_calls(monkeypatch):
    """The native planner's route (GpuExecutor.try_count_text -> prepare_planned):
    repeated calls are deduplicated into an alias segment applied on top of the
    compacted part's answers."""
    from pilosa_amd.models.view import VIEW_STANDARD
    from pilosa_amd.ops.device import GpuEngine
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    from tests.helpers import Env

    cpu = Env()
    try:
        cpu.create_index("i")
        f = cpu.field("i", "f")
        rng = np.random.default_rng(5)
        sizes = [60000, 30000, 9000, 8000, 7000, 6500, 6200, 6000] + [700, 300, 65, 64, 9, 1] * 2 + [40, 4, 2000, 1200]
        for r, k in enumerate(sizes):
            c = rng.choice(S * WIDTH, size=k, replace=False).astype(np.uint64)
            f.import_bits(np.full(k, r, np.uint64), c)
        gpu = GpuExecutor(cpu.holder, "cuda:0", executor=cpu.executor)
        shards = cpu.holder.index("i").available_shards()
        assert len(shards) == S
        dv = gpu.view_arena("i", "f", VIEW_STANDARD, shards)
        dv.HOTPAIR_ROWS = H
        dv.HOTPAIR_MIN_CONTAINERS = 0
        nrows = len(sizes)
        pairs = [(a, b) for a in range(H) for b in range(H) if a <= b]                 # 36 table-answered
        pairs += [(a, b) for a in range(H) for b in range(H, nrows)][:130]             # live
        pairs += [(b, 999) for b in (0, 9)] + [(10, 11), (11, 13), (12, 12)]            # an absent row, cold pairs
        uniq = len({(min(a, b), max(a, b)) for a, b in pairs})
        pairs = pairs + pairs[::3] + pairs[:20]                                        # repeated calls
        text = "\n".join(f"Count(Intersect(Row(f={a}), Row(f={b})))" for a, b in pairs)
        want = cpu.q("i", text)
        gpu.engine = _engine(gpu.engine.device)
        got = gpu.try_count_text("i", text, shards)
        print("counters", gpu.engine.ext.counts, "unique", uniq, "calls", len(pairs))
        assert got == want
        assert dv.hot_fresh()
        (nlive, nhot), = gpu.engine.ext.counts
        assert nhot == 36 and nlive + nhot == uniq < len(pairs)
        monkeypatch.setenv("PILOSA_PAIR_COMPACT", "0")
        gpu.engine = GpuEngine(gpu.engine.device)
        assert not gpu.engine.use_compact
        assert gpu.try_count_text("i", text, shards) == got
    finally:
        cpu.close()
