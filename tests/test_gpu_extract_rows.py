"""Extract(filter, Rows(field=)...) for set, time, mutex and bool fields on the
device (rows_extract_kernel, K28) against numpy and against the host path, on
the fixture of the TopK tests (tests/topk_util.py: it takes every branch of the
row traversal K28 shares with K25 -- three shards with a gap, keys 0, 7 and 15,
70 rows in all three encodings, lane-owned and cooperative arrays, a row at one
key only, ghost columns, row ids above 2^40) plus a mutex, a bool, a time and a
keyed set field (tests/extract_rows_util.py).  Every answer is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pilosa_amd import executor as executor_mod
from pilosa_amd.executor import Executor, ExtractedTable
from pilosa_amd.models.holder import Holder

from tests.extract_rows_util import FILTERS, GHOST, MX_IDS, ONE, T_IDS, RowsData, call_text, check
from tests.helpers import SW, Env
from tests.topk_util import A_IDS, SHARDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "PILOSA_EXTRACT_ROWS_WIDTH_CHILD"
SET_LIKE = ("a", "n", "mx", "b", "t")


@pytest.fixture(autouse=True)
def k28_on_and_no_fault(monkeypatch):
    """Every test asks for K28 itself, whatever the shipped default is, and
    no request may be answered by the host because the device failed."""
    monkeypatch.setenv("PILOSA_EXTRACT_ROWS_DEVICE", "1")
    f0 = executor_mod.DEVICE_FAULTS[0]
    yield
    assert executor_mod.DEVICE_FAULTS[0] == f0


@pytest.fixture(scope="module")
def envs():
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    env.data = RowsData()
    env.data.load(env)
    gpu = GpuExecutor(env.holder, "cuda:0", executor=env.executor)
    env.executor.gpu = gpu
    yield env, gpu
    env.close()


def _host(env, gpu, monkeypatch, q):
    """The same request with the device route declining: the host gather."""
    def decline(*a, **k):
        raise NotImplementedError
    with monkeypatch.context() as m:
        m.setattr(gpu, "bsi_extract", decline)
        st0 = gpu.stats()
        r = env.q1("i", q)
        st1 = gpu.stats()
        assert (st1["extractDevice"], st1["extractRowsDevice"]) == (st0["extractDevice"], st0["extractRowsDevice"])
    return r


def _device(env, gpu, q, rows=1, ints=0):
    """The request on the device: all local shards are one map step, so the
    counters rise by the fields of each kind."""
    st0, f0 = gpu.stats(), executor_mod.DEVICE_FAULTS[0]
    r = env.q1("i", q)
    st1 = gpu.stats()
    assert isinstance(r, ExtractedTable)
    assert executor_mod.DEVICE_FAULTS[0] == f0
    assert st1["extractRowsDevice"] == st0["extractRowsDevice"] + rows, "K28 did not answer"
    assert st1["extractDevice"] == st0["extractDevice"] + ints
    return r


def test_fixture_shape(envs):
    env, gpu = envs
    d = env.data
    v = gpu.view_arena("i", "a", "standard", list(SHARDS))
    assert v.D == 70 > 64 and int(v.rows[-1]) >= 1 << 40
    if SW >= 1 << 20:
        m = v.t_meta.cpu().numpy()
        assert set(((m >> 4) & 3).tolist()) >= {1, 2, 3}                  # 1 array, 2 bitmap, 3 run
        arr = (m >> 6 & 0x1FFFF)[((m >> 4) & 3) == 1]
        assert (arr <= 32).any() and (arr > 32).any() and (arr > 512).any()   # lane-owned and cooperative arrays
    if SW == 1 << 20:
        assert set(((d.cols % np.uint64(SW)) >> np.uint64(16)).tolist()) == {0, 7, 15}
        assert set(((d.cols[d.rows["a"][A_IDS[2]]] % np.uint64(SW)) >> np.uint64(16)).tolist()) == {7}
    mx = gpu.view_arena("i", "mx", "standard", list(SHARDS))
    assert mx.rows.tolist() == sorted(MX_IDS) and len(MX_IDS) == 5
    assert np.sum([m for m in d.more["mx"].values()], axis=0).max() == 1     # every column in at most one row
    assert all(m.any() for rows in d.more.values() for m in rows.values())
    ghosts = d.cols[d.mask(GHOST)]
    assert len(ghosts) == 40 * len(SHARDS) and not d.exists[d.mask(GHOST)].any()
    assert d.cells("a", np.sort(ghosts)) == [[A_IDS[4]]] * len(ghosts)       # they hold exactly that row
    assert d.cells("mx", np.sort(ghosts)).count(None) not in (0, len(ghosts))
    assert d.columns(ONE).tolist() == [d.one_col] and d.one_col // SW == SHARDS[-1]
    assert len(d.cells("a", d.columns(ONE))[0]) > 1
    tf = env.holder.field("i", "t")
    assert tf.time_quantum() == "YMD" and len(tf.views) > 1 and max(T_IDS) > 1 << 40
    assert env.holder.field("i", "ks").options.keys


@pytest.mark.parametrize("filt", FILTERS)
def test_device_equals_numpy_and_host(envs, monkeypatch, filt):
    env, gpu = envs
    d = env.data
    columns = d.columns(filt)
    for field in SET_LIKE:
        q = call_text(filt, (field,))
        got = _device(env, gpu, q)
        check(d, got, (field,), columns)
        assert _host(env, gpu, monkeypatch, q) == got, q
    q = call_text(filt, SET_LIKE)
    got = _device(env, gpu, q, rows=len(SET_LIKE))
    check(d, got, SET_LIKE, columns)
    assert _host(env, gpu, monkeypatch, q) == got, q


def test_only_set_like_fields_run_on_the_device(envs):
    env, gpu = envs
    d = env.data
    l0 = gpu.stats()["extractRowsLaunches"]
    got = _device(env, gpu, call_text("Row(f=1)", ("a", "t")), rows=2)
    check(d, got, ("a", "t"), d.columns("Row(f=1)"))
    assert gpu.stats()["extractRowsLaunches"] == l0 + 4        # a count and a fill pass per list field
    cells = got.cells(0)
    assert [] in cells and any(len(c) > 5 for c in cells)


def test_int_set_and_mutex_fields_in_one_call(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    q = call_text("Row(f=1)", ("w", "a", "mx"))
    env.q1("i", q)                                   # the arenas are resident from here on
    st0 = gpu.stats()
    got = _device(env, gpu, q, rows=2, ints=1)
    st1 = gpu.stats()
    assert st1["launches"] == st0["launches"] + 2    # one count pass, one K27 pass: K28 does not count here
    assert st1["extractRowsLaunches"] == st0["extractRowsLaunches"] + 3   # count, fill; scalar
    check(d, got, ("w", "a", "mx"), d.columns("Row(f=1)"))
    assert _host(env, gpu, monkeypatch, q) == got


@pytest.mark.parametrize("rpb", ["0", "64", "1"])
def test_rows_per_workgroup(envs, monkeypatch, rpb):
    """One workgroup per (shard, key) for all 70 rows, chunks of 64 (a last
    chunk of 6) and one row per workgroup -- there only the sort makes a
    column's rows ascending."""
    env, gpu = envs
    d = env.data
    monkeypatch.setenv("PILOSA_EXTRACT_ROWS_PER_BLOCK", rpb)
    for filt in ("Row(f=1)", "Not(Row(f=1))"):
        check(d, _device(env, gpu, call_text(filt, ("a", "mx")), rows=2), ("a", "mx"), d.columns(filt))


@pytest.mark.parametrize("rpw", ["16", "32", "64"])
def test_rows_per_wave_step(envs, monkeypatch, rpw):
    env, gpu = envs
    d = env.data
    monkeypatch.setenv("PILOSA_EXTRACT_ROWS_PER_WAVE", rpw)
    for filt in ("Row(f=1)", "Intersect(Row(f=1), Row(g=1))"):
        check(d, _device(env, gpu, call_text(filt, ("a", "b")), rows=2), ("a", "b"), d.columns(filt))


def test_without_keymask(envs, monkeypatch):
    """A view without the key-presence table: the meta walk finds the containers."""
    env, gpu = envs
    d = env.data
    v = gpu.view_arena("i", "a", "standard", list(SHARDS))
    monkeypatch.setenv("PILOSA_KEYMASK", "0")
    saved = getattr(v, "_keymask", None)
    v._keymask = None
    try:
        assert int(v.viewdev()["keymask"]) == 0
        for filt in ("Row(f=1)", "Row(w > 500)"):
            check(d, _device(env, gpu, call_text(filt, ("a",))), ("a",), d.columns(filt))
        assert int(v.viewdev()["keymask"]) == 0
    finally:
        v._keymask = saved


def test_windows(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    columns = d.columns("Row(f=1)")
    n = len(columns)
    # a column in the middle of a 32-column word that holds a later column too: the window ends mid-word
    mid = next(k for k in range(10, n - 1) if 8 <= int(columns[k]) % 32 <= 20
               and int(columns[k + 1]) // 32 == int(columns[k]) // 32)
    in_word = mid + 1
    key0 = int(np.searchsorted(columns, min(SW, 1 << 16)))          # ends exactly on a (shard, key) boundary
    shard0 = int(np.searchsorted(columns, SW))                      # ... and on a shard boundary
    last = int(np.searchsorted(columns, SHARDS[-1] * SW))           # starts in the last shard
    assert 0 < in_word < key0 <= shard0 < last < n - 5
    cases = [(0, in_word), (7, in_word - 7), (0, key0), (3, key0 - 3), (key0, 40), (0, shard0), (shard0 - 1, 2),
             (last + 2, 3), (last + 2, None), (n - 1, 5), (n, 5), (n + 3, None), (0, 0), (0, 1), (0, n), (5, None)]
    fields = ("a", "mx", "t")
    for off, lim in cases:
        q = call_text("Row(f=1)", fields, offset=off, limit=lim)
        got = _device(env, gpu, q, rows=3)
        want = columns[off:] if lim is None else columns[off:off + lim]
        check(d, got, fields, want)       # offsets[-1] == len(rows); no entry of a column beyond the window
        assert _host(env, gpu, monkeypatch, q) == got, (off, lim)


def test_knobs(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    columns = d.columns("Row(f=1)")
    q = call_text("Row(f=1)", ("a", "w", "mx"))
    want = _device(env, gpu, q, rows=2, ints=1)
    check(d, want, ("a", "w", "mx"), columns)
    with monkeypatch.context() as m:     # set-like fields on the host, the int field still on K27
        m.setenv("PILOSA_EXTRACT_ROWS_DEVICE", "0")
        assert _device(env, gpu, q, rows=0, ints=1) == want
    with monkeypatch.context() as m:     # everything on the host
        m.setenv("PILOSA_EXTRACT_DEVICE", "0")
        assert _device(env, gpu, q, rows=0, ints=0) == want
    with monkeypatch.context() as m:     # more entries than allowed: the set field alone goes to the host
        m.setenv("PILOSA_EXTRACT_ROWS_MAX_ENTRIES", "10")
        assert _device(env, gpu, q, rows=1, ints=1) == want
        m.setenv("PILOSA_EXTRACT_ROWS_MAX_ENTRIES", str(1 << 30))
        assert _device(env, gpu, q, rows=2, ints=1) == want


def test_keyed_field_returns_keys(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    q = "Extract(Row(f=1), Rows(field=ks), limit=40)"
    got = _device(env, gpu, q)
    assert got.fields == [("ks", "[]string")]
    assert got.cells(0) == d.cells("ks", d.columns("Row(f=1)")[:40]) and sum(map(len, got.cells(0))) == 10
    assert _host(env, gpu, monkeypatch, q) == got


def test_after_writes():
    """After device writes: a bit in a new row (the dense row count grows), a
    bit cleared, a mutex column moved to another row."""
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env(gpu=lambda h: GpuExecutor(h, "cuda:0"))
    try:
        gpu = env.executor.gpu
        gpu.executor = env.executor
        env.create_index("i")
        env.field("i", "f")
        env.field("i", "a")
        env.field("i", "mx", type="mutex")
        rng = np.random.default_rng(5)
        cols = np.sort(np.concatenate([s * SW + rng.choice(SW // 2, 3000, replace=False) for s in SHARDS]))
        cols = cols.astype(np.uint64)
        idx = env.holder.index("i")
        idx.field("f").import_bits(np.ones(len(cols), np.uint64), cols)
        member = {r: rng.random(len(cols)) < p for r, p in ((1, 0.5), (4, 0.1), (9, 0.01))}
        for r, m in member.items():
            idx.field("a").import_bits(np.full(int(m.sum()), r, np.uint64), cols[m])
        mrow = rng.integers(0, 4, len(cols))
        idx.field("mx").import_bits(mrow.astype(np.uint64), cols)
        a = {int(c): [r for r in sorted(member) if member[r][k]] for k, c in enumerate(cols.tolist())}
        mx = dict(zip(cols.tolist(), mrow.tolist()))
        q = "Extract(Row(f=1), Rows(field=a), Rows(field=mx))"

        def check_now():
            got = _device(env, gpu, q, rows=2)
            assert got.columns.tolist() == sorted(a)
            assert got.cells(0) == [a[c] for c in sorted(a)] and got.cells(1) == [mx.get(c) for c in sorted(a)]
        check_now()
        D0 = gpu.view_arena("i", "a", "standard", list(SHARDS)).D
        c1 = int(cols[10])
        env.q("i", f"Set({c1}, a=7)")                       # a new row between the old ones
        a[c1] = sorted(a[c1] + [7])
        check_now()
        assert gpu.view_arena("i", "a", "standard", list(SHARDS)).D == D0 + 1
        c2 = next(c for c in sorted(a, reverse=True) if 1 in a[c])
        env.q("i", f"Clear({c2}, a=1)")
        a[c2].remove(1)
        check_now()
        c3 = int(cols[-20])
        env.q("i", f"Set({c3}, mx={(mx[c3] + 1) % 4})")     # the mutex moves the column to another row
        mx[c3] = (mx[c3] + 1) % 4
        check_now()
        new = SW + SW // 2 + 9                              # a new column of the filter, in no row
        assert new not in a
        env.q("i", f"Set({new}, f=1)")
        a[new] = []
        check_now()
    finally:
        env.close()


def test_lazily_opened_holder_stays_cold():
    import shutil
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    data = RowsData()
    data.load(env)
    env.holder.close()
    holder = Holder(env.dir, lazy_fragments=True).open()
    gpu = GpuExecutor(holder, "cuda:0")
    ex = Executor(holder, gpu=gpu)
    gpu.executor = ex
    try:
        for field in ("a", "mx"):
            n0 = gpu.stats()["extractRowsDevice"]
            r = ex.execute("i", call_text("Row(f=1)", (field,))).results[0]
            assert gpu.stats()["extractRowsDevice"] == n0 + 1
            check(data, r, (field,), data.columns("Row(f=1)"))
            frags = holder.view("i", field, "standard").all_fragments()
            assert frags and all(f.is_cold() for f in frags), "Extract read a standard fragment on the host"
    finally:
        ex.close()
        holder.close()
        env.executor.close()
        shutil.rmtree(env.dir, ignore_errors=True)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("exp", [16, 22])
def test_shard_widths(exp):
    """This file again in a fresh interpreter at another shard width (the
    width is fixed per process): one container key per shard at 2^16, four
    device sub-shards per shard at 2^22."""
    if os.environ.get(CHILD):
        return   # the child runs every other test of the file, never this one again
    env = dict(os.environ, PILOSA_SHARD_WIDTH=str(exp))
    env[CHILD] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "--timeout", "300", "--timeout-method", "thread", "-k", "not test_shard_widths",
                        "tests/test_gpu_extract_rows.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
