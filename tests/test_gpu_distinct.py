"""Distinct(field=) on the device (bsi_distinct_kernel, K26) against numpy and
against the host path, on the smallest shapes at which the kernel can go wrong:
three shards with a gap, containers at keys 0, 7 and 15, all three container
encodings, values that occur only at a slot boundary (columns 8191 and 8192 of
a key) or in one column, a non-zero base, a field deep enough that its planes
are staged by every wave several times, and a depth-40 field the host answers.
Every answer is an exact set of integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pilosa_amd.executor import Executor, SignedRow
from pilosa_amd.models.holder import Holder

from tests.distinct_util import call_text, considered, filters, flat, load, oracle, standard_rows
from tests.helpers import SW, Env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARDS = (0, 1, 3)
U = SW // 16          # columns per sixteenth of a shard (one container key at 2^20)
CHILD = "PILOSA_DISTINCT_WIDTH_CHILD"
BIG_RUN = (1 << 38) + 5
# values held by exactly one column each: at offsets 8191 and 8192 of shard 0
# (the last column of tile slot 0 and the first of slot 1) and once in the last shard
EDGE = {"v": (1991, -1993, 1997), "w": (1091, 1093, 1097), "m": (1 << 20, -(1 << 20), 777777)}
RUN = {"v": -37, "w": 612, "m": -(1 << 19) - 5, "big": BIG_RUN}


class Data:
    """Per shard: 10,000 consecutive columns with random values from a pool of
    40 from offset 100 (bitmap planes), 10,000 consecutive columns holding one
    value from key 7 (run containers; every column after the first finds its
    value already marked) and 300 scattered columns in key 15 (arrays).
    v: +-2000 (depth 11); w: base 100, every 5th column without a value;
    m: depth 21, magnitudes up to 2^20, a random 45% of the random stretch
    without a value (so its exists row is a bitmap there: too many runs for a
    run container, too many columns for an array); big: depth 40."""
    schema = {"v": dict(min=-2000, max=2000), "w": dict(min=100, max=1100, base=100),
              "m": dict(min=-(1 << 20), max=1 << 20), "big": dict(min=-(1 << 39), max=1 << 39)}

    def __init__(self, seed=29):
        rng = np.random.default_rng(seed)
        pool = {"v": np.unique(np.concatenate([[-2000, -1, 0, 1, 2000], rng.integers(-1900, 1901, 35)])),
                "w": np.unique(rng.integers(100, 1001, 40)),
                "m": np.unique(np.concatenate([[-(1 << 20) + 1, (1 << 20) - 1, 0],
                                               rng.integers(-(1 << 20) + 1, 1 << 20, 37)]))}
        cols = []
        vals = {k: [] for k in self.schema}
        for s in SHARDS:
            a = s * SW + 100 + np.arange(10000)
            b = s * SW + 7 * U + 50 + np.arange(10000)
            c = s * SW + 15 * U + np.sort(rng.choice(min(U - 1, 40000), 300, replace=False))
            cols += [a, b, c]
            for k in ("v", "w", "m"):
                vals[k] += [rng.choice(pool[k], 10000), np.full(10000, RUN[k]), rng.choice(pool[k], 300)]
            vals["big"] += [rng.integers(-(1 << 20), 1 << 20, 10000), np.full(10000, BIG_RUN),
                            np.concatenate([[-(1 << 39), 1 << 39], rng.integers(-(1 << 39) + 1, 1 << 39, 298)])]
        self.cols = np.concatenate(cols).astype(np.uint64)
        assert len(np.unique(self.cols)) == len(self.cols)
        n = len(self.cols)
        self.vals = {k: np.concatenate(v).astype(np.int64) for k, v in vals.items()}
        self.special = [int(np.flatnonzero(self.cols == c)[0]) for c in (8191, 8192, SHARDS[-1] * SW + 5100)]
        self.has = {k: np.ones(n, bool) for k in self.schema}
        self.has["w"] = np.arange(n) % 5 != 0
        stretch_a = (self.cols % np.uint64(SW) >= 100) & (self.cols % np.uint64(SW) < 10100)
        self.has["m"] = ~stretch_a | (rng.random(n) < 0.55)
        for k, edge in EDGE.items():
            assert not np.isin(edge, pool[k]).any() and RUN[k] not in edge
            self.vals[k][self.special] = edge
            self.has[k][self.special] = True
        self.extra = np.array([s * SW + 3 * U + 7 for s in SHARDS], np.uint64)   # exist, hold no value
        self.rows = standard_rows(self, rng)
        self.rows[1][self.special] = True    # the one-column values stay inside Row(f=1)


@pytest.fixture(scope="module")
def envs():
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    env.data = Data()
    load(env, env.data)
    gpu = GpuExecutor(env.holder, "cuda:0", executor=env.executor)
    env.executor.gpu = gpu
    yield env, gpu
    env.close()


def _arena_encodings(gpu, field):
    dv = gpu.view_arena("i", field, "bsig_" + field, list(SHARDS))
    m = dv.t_meta
    m = m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)
    return dv, m


def _row_metas(dv, m, d):
    """Container metadata words of dense row d of an arena over all its shards."""
    rp = dv.t_rowptr
    rp = (rp.cpu().numpy() if hasattr(rp, "cpu") else np.asarray(rp)).reshape(dv.S, dv.D + 1).astype(np.int64)
    sb = dv.t_shard_base
    sb = (sb.cpu().numpy() if hasattr(sb, "cpu") else np.asarray(sb)).astype(np.int64)
    return np.concatenate([m[sb[s] + rp[s, d]:sb[s] + rp[s, d + 1]] for s in range(dv.S)])


def _encodings_of_row(dv, m, d):
    return set(((_row_metas(dv, m, d) >> 4) & 3).tolist())


def test_fixture_holds_every_container_encoding(envs):
    """1 array, 2 bitmap, 3 run, among the planes and in the exists rows the
    kernel stages: v's exists row is runs (the stretches) and arrays (the
    scattered columns), m's -- a random 45% of the random stretch missing -- a
    bitmap there; v's planes are bitmaps (random stretch), runs (constant stretch) and
    arrays."""
    env, gpu = envs
    d = env.data
    depth = {n: env.holder.field("i", n).bsi_group(n).bit_depth for n in d.schema}
    assert depth == {"v": 11, "w": 10, "m": 21, "big": 40}
    assert env.holder.field("i", "w").bsi_group("w").base == 100
    assert sorted(set((d.cols // np.uint64(SW)).tolist())) == list(SHARDS)
    if SW >= 1 << 20:
        exists, planes = set(), set()
        for field in ("v", "w", "m"):
            dv, m = _arena_encodings(gpu, field)
            assert set(((m >> 4) & 3).tolist()) >= {1, 2, 3}, field
            exists |= _encodings_of_row(dv, m, dv.dense(0))
            for i in range(depth[field]):
                planes |= _encodings_of_row(dv, m, dv.dense(2 + i))
        assert exists >= {1, 2, 3} and planes >= {1, 2, 3}
    if SW == 1 << 20:   # containers at keys 0, 7 and 15 of every shard
        dv, m = _arena_encodings(gpu, "v")
        assert set((_row_metas(dv, m, dv.dense(0)) & 15).tolist()) == {0, 7, 15}
    for k, edge in EDGE.items():
        for x in edge:
            assert int((d.vals[k][d.has[k]] == x).sum()) == 1
    assert d.cols[d.special[0]] == 8191 and d.cols[d.special[1]] == 8192
    assert d.cols[d.special[2]] // np.uint64(SW) == SHARDS[-1]


def _host(env, gpu, monkeypatch, q):
    """The same request with the device route declining: Fragment.distinct."""
    def decline(*a, **k):
        raise NotImplementedError
    with monkeypatch.context() as m:
        m.setattr(gpu, "bsi_distinct", decline)
        n0 = gpu.stats()["distinctDevice"]
        r = env.q1("i", q)
        assert gpu.stats()["distinctDevice"] == n0
    return flat(r)


def _device(env, gpu, q):
    st0 = gpu.stats()
    r = env.q1("i", q)
    st1 = gpu.stats()
    assert isinstance(r, SignedRow)
    # all local shards are one map step
    assert st1["distinctDevice"] == st0["distinctDevice"] + 1, "the device pass did not answer"
    return flat(r)


@pytest.mark.parametrize("field", ["v", "w", "m"])
def test_device_equals_numpy_and_host(envs, monkeypatch, field):
    env, gpu = envs
    d = env.data
    fl = filters(d, other="v" if field == "w" else "w", bound=10 if field == "w" else 500)
    assert len(fl) == 10
    for filt, mask in fl:
        q = call_text(field, filt)
        want = oracle(considered(d, field, mask))
        assert _device(env, gpu, q) == want, q
        assert _host(env, gpu, monkeypatch, q) == want, q
    # the slot-boundary and one-column values are in the unfiltered answer
    pos, neg = _device(env, gpu, call_text(field))
    for x in EDGE[field]:
        assert (x in pos) if x >= 0 else (-x in neg), x
    assert len(pos) + len(neg) > 40


def test_one_launch_per_call(envs):
    env, gpu = envs
    st0 = gpu.stats()
    env.q1("i", "Distinct(field=v)")
    st1 = gpu.stats()
    assert st1["distinctDevice"] == st0["distinctDevice"] + 1 and st1["launches"] == st0["launches"] + 1


def test_deep_field_is_answered_by_the_host(envs):
    env, gpu = envs
    d = env.data
    for filt, mask in filters(d)[:2]:
        n0 = gpu.stats()["distinctDevice"]
        assert flat(env.q1("i", call_text("big", filt))) == oracle(considered(d, "big", mask))
        assert gpu.stats()["distinctDevice"] == n0
    assert 1 << 39 in flat(env.q1("i", "Distinct(field=big)"))[0]


def test_slots_knob_and_its_clamp(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    ext = gpu.engine.ext
    # (2 + depth) * n KiB next to 40 KiB of wave scratch inside 160 KiB
    assert [ext.distinct_slots(11, n) for n in (0, 1, 2, 4, 8)] == [8, 1, 2, 4, 8]
    assert [ext.distinct_slots(21, n) for n in (0, 1, 2, 4, 8)] == [4, 1, 2, 4, 4]
    assert [ext.distinct_slots(26, n) for n in (0, 1, 2, 4, 8)] == [4, 1, 2, 4, 4]
    assert ext.distinct_slots(13, 8) == 8 and ext.distinct_slots(14, 8) == 4 and ext.distinct_slots(30, 8) == 2
    assert ext.distinct_slots(11, 3) == 2 and ext.distinct_slots(11, 100) == 8
    for field in ("v", "m"):
        for filt, mask in filters(d)[:2]:
            want = oracle(considered(d, field, mask))
            for n in ("1", "2", "4", "8"):
                monkeypatch.setenv("PILOSA_DISTINCT_SLOTS", n)
                assert _device(env, gpu, call_text(field, filt)) == want, (field, filt, n)


def test_marking_variants_agree(envs):
    """The always-OR baseline and the previous-value skip mark what the
    shipped test-first variant marks."""
    env, gpu = envs
    d = env.data
    bv = gpu.view_arena("i", "m", "bsig_m", list(SHARDS))
    want_pos, want_neg = oracle(d.vals["m"][d.has["m"]])
    for mark in (0, 1, 2):
        pos, neg = gpu.engine.bsi_distinct(None, bv, 21, 2, mark)
        assert (pos.tolist(), neg.tolist()) == (want_pos, want_neg), mark


def test_max_depth_knob_sends_the_field_to_the_host(envs, monkeypatch):
    env, gpu = envs
    want = oracle(env.data.vals["v"])
    monkeypatch.setenv("PILOSA_DISTINCT_MAX_DEPTH", "10")      # v is depth 11
    n0 = gpu.stats()["distinctDevice"]
    assert flat(env.q1("i", "Distinct(field=v)")) == want
    assert gpu.stats()["distinctDevice"] == n0
    monkeypatch.setenv("PILOSA_DISTINCT_MAX_DEPTH", "11")
    assert _device(env, gpu, "Distinct(field=v)") == want
    monkeypatch.setenv("PILOSA_DISTINCT_MAX_DEPTH", "31")      # outside 1..30: the default, 26
    n0 = gpu.stats()["distinctDevice"]
    assert flat(env.q1("i", "Distinct(field=big)")) == oracle(env.data.vals["big"])
    assert gpu.stats()["distinctDevice"] == n0


def test_device_knob_off_sends_everything_to_the_host(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    monkeypatch.setenv("PILOSA_DISTINCT_DEVICE", "0")
    n0 = gpu.stats()["distinctDevice"]
    for field in ("v", "w", "m"):
        assert flat(env.q1("i", call_text(field, "Row(f=1)"))) == oracle(considered(d, field, d.rows[1]))
    assert gpu.stats()["distinctDevice"] == n0


def test_after_writes():
    """Overwriting the only column of a value with a common one makes the value
    vanish; a value beyond the current bit depth appears, with the new planes."""
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env(gpu=lambda h: GpuExecutor(h, "cuda:0"))
    try:
        gpu = env.executor.gpu
        gpu.executor = env.executor
        env.create_index("i")
        env.field("i", "v", type="int", min=-100000, max=100000)
        rng = np.random.default_rng(3)
        cols = np.concatenate([s * SW + rng.choice(SW // 2, 3000, replace=False) for s in SHARDS])
        vals = rng.choice(rng.integers(-900, 901, 30), len(cols))
        once_col = int(cols[-1])
        vals[-1] = 1001
        env.holder.index("i").field("v").import_values(cols.astype(np.uint64), vals)
        cur = dict(zip(cols.tolist(), vals.tolist()))
        depth0 = env.holder.field("i", "v").bsi_group("v").bit_depth
        assert depth0 == 10
        assert _device(env, gpu, "Distinct(field=v)") == oracle(list(cur.values()))
        common = int(vals[0])
        env.q("i", f"Set({once_col}, v={common})")
        cur[once_col] = common
        got = _device(env, gpu, "Distinct(field=v)")
        assert got == oracle(list(cur.values())) and 1001 not in got[0]
        new_col = SW + SW // 2 + 9
        env.q("i", f"Set({new_col}, v=-70000)")
        cur[new_col] = -70000
        assert env.holder.field("i", "v").bsi_group("v").bit_depth == 17 > depth0
        got = _device(env, gpu, "Distinct(field=v)")
        assert got == oracle(list(cur.values())) and 70000 in got[1]
    finally:
        env.close()


def test_lazily_opened_holder_stays_cold():
    import shutil
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    data = Data()
    load(env, data)
    env.holder.close()
    holder = Holder(env.dir, lazy_fragments=True).open()
    gpu = GpuExecutor(holder, "cuda:0")
    ex = Executor(holder, gpu=gpu)
    gpu.executor = ex
    try:
        for field, (filt, mask) in (("m", filters(data)[0]), ("v", filters(data)[1])):
            n0 = gpu.stats()["distinctDevice"]
            r = ex.execute("i", call_text(field, filt)).results[0]
            assert gpu.stats()["distinctDevice"] == n0 + 1
            assert flat(r) == oracle(considered(data, field, mask))
            frags = holder.view("i", field, "bsig_" + field).all_fragments()
            assert frags and all(f.is_cold() for f in frags), "Distinct read a BSI fragment on the host"
    finally:
        ex.close()
        holder.close()
        env.executor.close()
        shutil.rmtree(env.dir, ignore_errors=True)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("exp", [16, 22])
def test_shard_widths(exp):
    """This file again in a fresh interpreter at another shard width (the
    width is fixed per process): one container key per shard at 2^16, so only
    the first tile slots are filled; four device sub-shards per shard at 2^22."""
    if os.environ.get(CHILD):
        return   # the child runs every other test of the file, never this one again
    env = dict(os.environ, PILOSA_SHARD_WIDTH=str(exp))
    env[CHILD] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "--timeout", "300", "--timeout-method", "thread", "-k", "not test_shard_widths",
                        "tests/test_gpu_distinct.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
