"""Extract(filter, Rows(field=)...) on the device (bsi_extract_kernel, K27)
against numpy and against the host path, on the smallest shapes at which the
kernel can go wrong: the fixture of tests/test_gpu_distinct.py (three shards
with a gap, containers at keys 0, 7 and 15, all three container encodings)
plus the first and last column of a shard, filter columns on both sides of a
slot boundary (offsets 8191 / 8192 of a key) and of a wave boundary of the
block scan (2047 / 2048 of a slot), a fully set 32-column word, a filter of
one column in the last shard, columns without a value between columns with
one, and fields of depth 11, 21 and 32.  Every answer is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import Executor, ExtractedTable
from pilosa_amd.models.holder import Holder

from tests.distinct_util import load
from tests.extract_util import call_text, check_ints, filters, int_cells, window
from tests.helpers import SW, Env
from tests.test_gpu_distinct import SHARDS, Data as DistinctData, _arena_encodings, _encodings_of_row

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "PILOSA_EXTRACT_WIDTH_CHILD"
LAST = SHARDS[-1] * SW + SW - 1
EDGES = (0, SW - 1, LAST)              # first and last column of a shard
PINNED = (2047, 2048, 8191, 8192)      # wave boundary of the scan, slot boundary
WORD = 4096 + np.arange(32)            # one whole 32-column word
M32 = (1 << 32) - 1


class Data(DistinctData):
    """tests/test_gpu_distinct.py's fixture, and: d32, a depth-32 field
    (magnitudes up to 2^32 - 1, a third of the columns without a value); the
    columns EDGES with a value everywhere; PINNED, WORD and EDGES inside
    Row(f=1); Row(f=6) = the last column of the last shard alone."""
    def __init__(self, seed=29):
        super().__init__(seed)
        self.schema = dict(DistinctData.schema, d32=dict(min=-M32, max=M32))
        rng = np.random.default_rng(seed + 1)
        n = len(self.cols)
        self.vals["d32"] = rng.integers(-M32, M32 + 1, n).astype(np.int64)
        self.vals["d32"][:4] = [M32, -M32, 0, 1 << 31]
        self.has["d32"] = rng.random(n) < 0.67
        self.has["d32"][:4] = True
        k = len(EDGES)
        self.cols = np.concatenate([self.cols, np.array(EDGES, np.uint64)])
        for f, new in (("v", (5, -6, 7)), ("w", (105, 106, 107)), ("m", (-8, 9, 10)), ("big", (11, -12, 13)),
                       ("d32", (M32, -14, -M32))):
            self.vals[f] = np.concatenate([self.vals[f], np.array(new, np.int64)])
            self.has[f] = np.concatenate([self.has[f], np.ones(k, bool)])
        for r in self.rows:
            self.rows[r] = np.concatenate([self.rows[r], np.zeros(k, bool)])
        self.rows[1][-k:] = True
        self.rows[1][np.isin(self.cols, np.concatenate([PINNED, WORD]).astype(np.uint64))] = True
        self.rows[2] = self.has["v"] & (self.vals["v"] < 0)
        self.rows[3] = self.has["v"] & (self.vals["v"] >= 0)
        self.rows[6] = self.cols == np.uint64(LAST)


def set_cells(d, columns):
    """The oracle's rows of set field f per column."""
    member = {int(c): [] for c in columns.tolist()}
    for r in sorted(d.rows):
        cs = d.cols[d.rows[r]]
        if r == 1:
            cs = np.concatenate([cs, d.extra])
        for c in cs.tolist():
            if c in member:
                member[c].append(r)
    return [member[int(c)] for c in columns.tolist()]


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


def test_fixture(envs):
    env, gpu = envs
    d = env.data
    depth = {n: env.holder.field("i", n).bsi_group(n).bit_depth for n in d.schema}
    assert depth == {"v": 11, "w": 10, "m": 21, "big": 40, "d32": 32}
    assert env.holder.field("i", "w").bsi_group("w").base == 100
    f1 = dict(filters(d))["Row(f=1)"]
    assert np.isin(np.concatenate([PINNED, WORD, EDGES]).astype(np.uint64), f1).all()
    assert np.isin(d.extra, f1).all() and not np.isin(d.extra, d.cols).any()
    # nulls between values: m lacks a random 45% of the stretch Row(f=1) covers
    cells = int_cells(d, "m", f1)
    assert any(a is None and b is not None and c is not None for a, b, c in zip(cells[1:], cells, cells[2:]))
    assert dict(filters(d) + [("Row(f=6)", d.cols[d.rows[6]])])["Row(f=6)"].tolist() == [LAST]
    if SW >= 1 << 20:
        planes, rows = set(), set()
        for field in ("v", "m", "d32"):
            dv, m = _arena_encodings(gpu, field)
            rows |= _encodings_of_row(dv, m, dv.dense(0))
            for i in range(depth[field]):
                planes |= _encodings_of_row(dv, m, dv.dense(2 + i))
        assert rows >= {1, 2, 3} and planes >= {1, 2, 3}
        dv = gpu.view_arena("i", "f", "standard", list(SHARDS))
        mm = dv.t_meta
        mm = mm.cpu().numpy() if hasattr(mm, "cpu") else np.asarray(mm)
        assert _encodings_of_row(dv, mm, dv.dense(1)) >= {1, 2}      # the filter row: arrays and bitmaps


def _host(env, gpu, monkeypatch, q):
    """The same request with the device route declining: the host gather."""
    def decline(*a, **k):
        raise NotImplementedError
    with monkeypatch.context() as m:
        m.setattr(gpu, "bsi_extract", decline)
        n0 = gpu.stats()["extractDevice"]
        r = env.q1("i", q)
        assert gpu.stats()["extractDevice"] == n0
    return r


def _device(env, gpu, q, nfields=1):
    n0 = gpu.stats()["extractDevice"]
    r = env.q1("i", q)
    assert isinstance(r, ExtractedTable)
    # all local shards are one map step
    assert gpu.stats()["extractDevice"] == n0 + nfields, "the device pass did not answer"
    return r


@pytest.mark.parametrize("field", ["v", "w", "m", "d32"])
def test_device_equals_numpy_and_host(envs, monkeypatch, field):
    env, gpu = envs
    d = env.data
    fl = filters(d, other="v" if field == "w" else "w", bound=10 if field == "w" else 500)
    fl.append(("Row(f=6)", d.cols[d.rows[6]]))
    assert len(fl) == 8
    for filt, columns in fl:
        q = call_text(filt, (field,))
        got = _device(env, gpu, q)
        check_ints(d, got, (field,), columns)
        assert _host(env, gpu, monkeypatch, q) == got, q


def test_two_int_fields_and_a_set_field_in_one_call(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    for filt, columns in filters(d)[:3]:
        q = f"Extract({filt}, Rows(field=m), Rows(field=f), Rows(field=w))"
        env.q1("i", q)                                   # the arenas are resident from here on
        l0 = gpu.stats()["launches"]
        got = _device(env, gpu, q, nfields=2)
        assert gpu.stats()["launches"] == l0 + 3         # one count pass, one extract pass per int field
        assert got.fields == [("m", "int64"), ("f", "[]uint64"), ("w", "int64")]
        assert got.columns.tolist() == columns.tolist()
        assert got.cells(0) == int_cells(d, "m", columns) and got.cells(2) == int_cells(d, "w", columns)
        assert got.cells(1) == set_cells(d, columns)
        assert _host(env, gpu, monkeypatch, q) == got


def test_deep_field_is_answered_by_the_host(envs):
    env, gpu = envs
    d = env.data
    filt, columns = filters(d)[0]
    n0 = gpu.stats()["extractDevice"]
    check_ints(d, env.q1("i", call_text(filt, ("big",))), ("big",), columns)
    assert gpu.stats()["extractDevice"] == n0
    # next to a field the kernel takes, the deep one is gathered on the host over the device's columns
    got = _device(env, gpu, call_text(filt, ("big", "v")))
    check_ints(d, got, ("big", "v"), columns)
    assert 1 << 39 in got.cells(0) or -(1 << 39) in got.cells(0)


def test_slots_knob_and_its_clamp(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    ext = gpu.engine.ext
    # (3 + depth) * n KiB next to 40 KiB of wave scratch inside 160 KiB
    assert [ext.extract_slots(11, n) for n in (0, 1, 2, 4, 8)] == [8, 1, 2, 4, 8]
    assert [ext.extract_slots(21, n) for n in (0, 1, 2, 4, 8)] == [4, 1, 2, 4, 4]
    assert [ext.extract_slots(32, n) for n in (0, 1, 2, 4, 8)] == [2, 1, 2, 2, 2]
    assert ext.extract_slots(12, 8) == 8 and ext.extract_slots(13, 8) == 4 and ext.extract_slots(27, 8) == 4
    assert ext.extract_slots(28, 8) == 2 and ext.extract_slots(11, 3) == 2 and ext.extract_slots(11, 100) == 8
    for field in ("v", "m", "d32"):
        for filt, columns in filters(d)[:2]:
            for n in ("1", "2", "4", "8"):
                monkeypatch.setenv("PILOSA_EXTRACT_SLOTS", n)
                check_ints(d, _device(env, gpu, call_text(filt, (field,))), (field,), columns)


def test_device_knob_off_sends_everything_to_the_host(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    monkeypatch.setenv("PILOSA_EXTRACT_DEVICE", "0")
    n0 = gpu.stats()["extractDevice"]
    filt, columns = filters(d)[0]
    check_ints(d, env.q1("i", call_text(filt, ("v", "w", "m"))), ("v", "w", "m"), columns)
    assert gpu.stats()["extractDevice"] == n0


def test_windows(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    columns = dict(filters(d))["Row(f=1)"]
    n = len(columns)
    in_word = int(np.searchsorted(columns, 4096 + 10)) + 1          # ends mid-word (the fully set word)
    key0 = int(np.searchsorted(columns, min(SW, 1 << 16)))          # ends exactly on a (shard, key) boundary
    shard0 = int(np.searchsorted(columns, SW))                      # ... and on a shard boundary
    last = int(np.searchsorted(columns, SHARDS[-1] * SW))           # starts in the last shard
    assert 0 < in_word < key0 <= shard0 < last < n - 5
    cases = [(0, in_word), (7, in_word - 7), (0, key0), (3, key0 - 3), (key0, 40), (0, shard0), (shard0 - 1, 2),
             (last + 2, 3), (last + 2, None), (n - 1, 5), (n, 5), (n + 3, None), (0, 0), (0, 1), (0, n), (5, None)]
    for off, lim in cases:
        q = call_text("Row(f=1)", ("m", "f"), offset=off, limit=lim)
        got = _device(env, gpu, q)
        want = window(columns, off, lim)
        check_ints(d, got, ("m",), want)
        assert got.cells(1) == set_cells(d, want), (off, lim)
        assert _host(env, gpu, monkeypatch, q) == got, (off, lim)


def test_size_guard(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    columns = dict(filters(d))["Row(f=1)"]
    monkeypatch.setenv("PILOSA_EXTRACT_MAX_COLUMNS", "10")
    launched = []
    real = gpu.engine.ext.bsi_extract
    with monkeypatch.context() as m:
        m.setattr(gpu.engine, "ext", _Spy(gpu.engine.ext, "bsi_extract", launched))
        for q, k in ((call_text("Row(f=1)", ("v",)), len(columns)),
                     (call_text("Row(f=1)", ("v",), offset=8, limit=3), 11)):
            with pytest.raises(PilosaError) as e:
                env.q("i", q)
            assert str(e.value) == f"Extract(): {k} columns exceed the limit of 10; page with limit= and offset="
        assert not launched, "the guard ran after the extract pass"
        check_ints(d, _device(env, gpu, call_text("Row(f=1)", ("v",), offset=7, limit=3)), ("v",), columns[7:10])
        check_ints(d, _device(env, gpu, call_text("Row(f=6)", ("v",))), ("v",), np.array([LAST], np.uint64))
        assert launched
    assert gpu.engine.ext.bsi_extract is real


class _Spy:
    """The extension module with one function recording its calls."""

    def __init__(self, ext, name, log):
        self._ext, self._name, self._log = ext, name, log

    def __getattr__(self, k):
        fn = getattr(self._ext, k)
        if k != self._name:
            return fn

        def wrapped(*a, **kw):
            self._log.append(1)
            return fn(*a, **kw)
        return wrapped


def test_after_writes():
    """After device writes: a value changes, a value is cleared to null, a new
    column enters the filter."""
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env(gpu=lambda h: GpuExecutor(h, "cuda:0"))
    try:
        gpu = env.executor.gpu
        gpu.executor = env.executor
        env.create_index("i")
        env.field("i", "f")
        env.field("i", "v", type="int", min=-100000, max=100000)
        rng = np.random.default_rng(3)
        cols = np.sort(np.concatenate([s * SW + rng.choice(SW // 2, 3000, replace=False) for s in SHARDS]))
        vals = rng.integers(-900, 901, len(cols))
        idx = env.holder.index("i")
        idx.field("v").import_values(cols.astype(np.uint64), vals)
        idx.field("f").import_bits(np.ones(len(cols), np.uint64), cols.astype(np.uint64))
        cur = dict(zip(cols.tolist(), vals.tolist()))
        q = "Extract(Row(f=1), Rows(field=v))"

        def check():
            got = _device(env, gpu, q)
            assert got.columns.tolist() == sorted(cur) and got.cells(0) == [cur[c] for c in sorted(cur)]
        check()
        a, b = int(cols[10]), int(cols[-10])
        env.q("i", f"Set({a}, v=77777)")
        cur[a] = 77777
        check()
        env.q("i", f"Clear({b}, v={cur[b]})")
        cur[b] = None
        check()
        new = SW + SW // 2 + 9
        assert new not in cur
        env.q("i", f"Set({new}, f=1)")
        cur[new] = None
        check()
        env.q("i", f"Set({new}, v=-5)")
        cur[new] = -5
        check()
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
        for field, (filt, columns) in (("m", filters(data)[0]), ("v", filters(data)[1])):
            n0 = gpu.stats()["extractDevice"]
            r = ex.execute("i", call_text(filt, (field,))).results[0]
            assert gpu.stats()["extractDevice"] == n0 + 1
            check_ints(data, r, (field,), columns)
            frags = holder.view("i", field, "bsig_" + field).all_fragments()
            assert frags and all(f.is_cold() for f in frags), "Extract read a BSI fragment on the host"
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
                        "tests/test_gpu_extract.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
