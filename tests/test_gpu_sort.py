"""Sort(<filter>, field=, limit=, offset=, sort-desc=) on the device
(bsi_sort_select_kernel, K29, behind the bsi_kth descent) against numpy and
against the host path, on the smallest shapes at which the kernel can go wrong:
the fixture of tests/test_gpu_extract.py (three shards with a gap, containers
at keys 0, 7 and 15, all three container encodings, depths 10 / 11 / 21 / 32 /
40, base 100) plus one tie group per field whose members sit on both sides of
a wave boundary of the block scans (2047 / 2048 of a slot), of a slot boundary
(8191 / 8192 of a key), in a fully set 32-column word and in two more shards,
so that ``limit`` can cut the group at each of them.  Every answer is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import Executor, SortedColumns
from pilosa_amd.models.holder import Holder

from tests.distinct_util import filters, load
from tests.helpers import SW, Env
from tests.sort_util import call_text, check, cut_limits, oracle, tie_group, window
from tests.test_gpu_extract import LAST, M32, PINNED, SHARDS, WORD, Data as ExtractData, _Spy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "PILOSA_SORT_WIDTH_CHILD"
FIELDS = ("v", "w", "m", "d32")
# one column in each of the two other shards (inside the stretch of consecutive columns)
FAR = (SHARDS[1] * SW + 200, SHARDS[2] * SW + 200)
TIE_COLS = np.concatenate([PINNED, WORD, FAR]).astype(np.uint64)
TIE = {"v": 3, "w": 555, "m": -4242, "d32": -(1 << 31) - 7}


class Data(ExtractData):
    """tests/test_gpu_extract.py's fixture, and: the columns TIE_COLS hold
    TIE[field] in every field of FIELDS and sit inside Row(f=1); the two m
    values of magnitude 2^20 they displace (at 8191 / 8192) move next door."""
    def __init__(self, seed=29):
        super().__init__(seed)
        at = np.isin(self.cols, TIE_COLS)
        assert at.sum() == len(TIE_COLS)
        moved = np.isin(self.cols, np.array([8190, 8193], np.uint64))
        self.vals["m"][moved] = [1 << 20, -(1 << 20)]
        self.has["m"][moved] = True
        for f, t in TIE.items():
            self.vals[f][at] = t
            self.has[f][at] = True
        self.rows[1][at] = True
        self.rows[2] = self.has["v"] & (self.vals["v"] < 0)
        self.rows[3] = self.has["v"] & (self.vals["v"] >= 0)


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


def _filters(d, field):
    fl = filters(d, other="v" if field == "w" else "w", bound=10 if field == "w" else 500)
    return fl[:9] + [("Row(f=6)", d.rows[6])]


def _host(env, gpu, monkeypatch, q):
    """The same request with the device route declining: the host path."""
    def decline(*a, **k):
        raise NotImplementedError
    with monkeypatch.context() as m:
        m.setattr(gpu, "bsi_sort", decline)
        n0 = gpu.stats()["sortDevice"]
        r = env.q1("i", q)
        assert gpu.stats()["sortDevice"] == n0
    return r


def _device(env, gpu, q):
    n0 = gpu.stats()["sortDevice"]
    r = env.q1("i", q)
    assert isinstance(r, SortedColumns) and r.keys is None
    # all local shards are one map step
    assert gpu.stats()["sortDevice"] == n0 + 1, "the device pass did not answer"
    return r


def test_fixture(envs):
    env, gpu = envs
    d = env.data
    depth = {n: env.holder.field("i", n).bsi_group(n).bit_depth for n in d.schema}
    assert depth == {"v": 11, "w": 10, "m": 21, "big": 40, "d32": 32}
    assert env.holder.field("i", "w").bsi_group("w").base == 100
    for f in FIELDS:
        cols, vals = oracle(d, f, d.rows[1])
        lo, hi = tie_group(vals, TIE[f])
        # in column order inside the group: every pinned boundary can be cut
        assert hi - lo >= len(TIE_COLS) and np.isin(TIE_COLS, cols[lo:hi]).all(), f
        assert 0 < lo and hi < len(vals)
    assert len({int(c) // SW for c in TIE_COLS}) == 3
    assert d.cols[d.rows[6]].tolist() == [LAST]
    assert (d.vals["v"][d.rows[2]] < 0).all() and (d.vals["v"][d.rows[3]] >= 0).all()


@pytest.mark.parametrize("field", FIELDS)
def test_device_equals_numpy_and_host(envs, monkeypatch, field):
    """Every filter shape, both directions; the cut before, inside and after
    the largest tie group of each considered set."""
    env, gpu = envs
    d = env.data
    thresholds = set()
    for filt, mask in _filters(d, field):
        for desc in (False, True):
            want = oracle(d, field, mask, desc)
            n = len(want[0])
            lo, hi = tie_group(want[1], TIE[field])
            limits = [None, 1, (lo + hi) // 2, n + 1] if filt not in ("", "Row(f=1)") else \
                [None] + cut_limits(want[1], TIE[field])
            for k, lim in enumerate(limits):
                q = call_text(field, filt, limit=lim, desc=desc if (desc or k % 2) else None)
                got = _device(env, gpu, q)
                check(got, window(want, 0, lim), q)
                if lim is not None and 0 < lim < n:
                    thresholds.add(int(want[1][lim - 1]) - (100 if field == "w" else 0))
                if k < 3:
                    assert _host(env, gpu, monkeypatch, q) == got, q
    # the thresholds the descent returned: negative, positive (and 0 for v: the
    # smallest of Row(f=3)), the extremes of d32
    assert min(thresholds) < 0 < max(thresholds) or field == "w"
    if field == "v":
        assert 0 in thresholds
    if field == "d32":
        assert {M32, -M32} <= thresholds


def test_cuts_at_the_pinned_boundaries_and_offsets(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    for field in ("v", "d32"):
        for desc in (False, True):
            for filt, mask in (("", np.ones(len(d.cols), bool)), ("Row(f=1)", d.rows[1])):
                want = oracle(d, field, mask, desc)
                n = len(want[0])
                lo, hi = tie_group(want[1], TIE[field])
                group = want[0][lo:hi].tolist()
                # the cut right after 2047, 2048, the middle of the full word, 8191, 8192 and the first far column
                ends = [lo + group.index(int(c)) + 1 for c in (2047, 2048, 4096 + 15, 8191, 8192, FAR[0])]
                for lim in ends:
                    q = call_text(field, filt, limit=lim, desc=desc)
                    got = _device(env, gpu, q)
                    check(got, window(want, 0, lim), q)
                    assert int(got.values[-1]) == TIE[field]
                for off, lim in ((lo + 3, 40), (ends[2] - 5, 5), (5, None), (n - 2, 10), (n, 3), (n + 7, None),
                                 (lo, 0), (hi - 1, 2)):
                    q = call_text(field, filt, limit=lim, offset=off, desc=desc)
                    got = _device(env, gpu, q)
                    check(got, window(want, off, lim), q)
                    assert _host(env, gpu, monkeypatch, q) == got, q


def test_deep_field_is_answered_by_the_host(envs):
    env, gpu = envs
    d = env.data
    n0 = gpu.stats()["sortDevice"]
    for desc in (False, True):
        got = env.q1("i", call_text("big", "Row(f=1)", limit=50, desc=desc))
        check(got, window(oracle(d, "big", d.rows[1], desc), 0, 50))
    assert abs(int(env.q1("i", call_text("big", limit=1, desc=True)).values[0])) == 1 << 39
    assert gpu.stats()["sortDevice"] == n0


def test_slots_knob_and_its_clamp(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    ext = gpu.engine.ext
    # (2 + depth) * n KiB next to 40 KiB of wave scratch inside 160 KiB
    assert [ext.sort_slots(11, n) for n in (0, 1, 2, 4, 8)] == [8, 1, 2, 4, 8]
    assert [ext.sort_slots(21, n) for n in (0, 1, 2, 4, 8)] == [4, 1, 2, 4, 4]
    assert [ext.sort_slots(32, n) for n in (0, 1, 2, 4, 8)] == [2, 1, 2, 2, 2]
    assert ext.sort_slots(13, 8) == 8 and ext.sort_slots(14, 8) == 4 and ext.sort_slots(28, 8) == 4
    assert ext.sort_slots(29, 8) == 2 and ext.sort_slots(11, 3) == 2 and ext.sort_slots(11, 100) == 8
    assert ext.sort_blocks(3, 1) == 3 * 16 * 8 and ext.sort_blocks(3, 8) == 3 * 16
    for field in ("v", "m", "d32"):
        for desc in (False, True):
            want = oracle(d, field, d.rows[1], desc)
            lo, hi = tie_group(want[1], TIE[field])
            for lim in ((lo + hi) // 2, None):
                for n in ("1", "2", "4", "8"):
                    monkeypatch.setenv("PILOSA_SORT_SLOTS", n)
                    q = call_text(field, "Row(f=1)", limit=lim, desc=desc)
                    check(_device(env, gpu, q), window(want, 0, lim), (q, n))


def test_device_knob_off_sends_everything_to_the_host(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    monkeypatch.setenv("PILOSA_SORT_DEVICE", "0")
    n0 = gpu.stats()["sortDevice"]
    check(env.q1("i", call_text("v", "Row(f=1)", limit=100)), window(oracle(d, "v", d.rows[1]), 0, 100))
    assert gpu.stats()["sortDevice"] == n0


def test_launch_counter(envs):
    env, gpu = envs
    d = env.data
    n = len(oracle(d, "v", d.rows[1])[0])
    env.q1("i", call_text("v", "Row(f=1)", limit=5))       # the arenas are resident from here on
    l0 = gpu.stats()["launches"]
    _device(env, gpu, call_text("v", "Row(f=1)", limit=5))
    assert gpu.stats()["launches"] == l0 + 1 + 11 + 2      # init, one step per bit, count and fill
    l0 = gpu.stats()["launches"]
    _device(env, gpu, call_text("v", "Row(f=1)", limit=n))
    assert gpu.stats()["launches"] == l0 + 1 + 2           # everything is selected: no descent
    l0 = gpu.stats()["launches"]
    assert len(_device(env, gpu, call_text("v", "Row(f=9)", limit=5))) == 0
    assert gpu.stats()["launches"] <= l0 + 1


def test_size_guard(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    want = oracle(d, "v", d.rows[1])
    monkeypatch.setenv("PILOSA_SORT_MAX_COLUMNS", "10")
    launched = []
    real = gpu.engine.ext.bsi_sort_select
    with monkeypatch.context() as m:
        m.setattr(gpu.engine, "ext", _Spy(gpu.engine.ext, "bsi_sort_select", launched))
        for q, k in ((call_text("v", "Row(f=1)"), len(want[0])),
                     (call_text("v", "Row(f=1)", offset=8, limit=3), 11)):
            with pytest.raises(PilosaError) as e:
                env.q("i", q)
            assert str(e.value) == f"Sort(): {k} columns exceed the limit of 10; page with limit= and offset="
        assert not launched, "the guard ran after the selection pass"
        check(_device(env, gpu, call_text("v", "Row(f=1)", offset=7, limit=3)), window(want, 7, 3))
        check(_device(env, gpu, call_text("v", "Row(f=6)")), oracle(d, "v", d.rows[6]))
        assert launched
    assert gpu.engine.ext.bsi_sort_select is real


def test_after_writes():
    """After device writes: a value that enters the top k, and one that leaves it."""
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

        def check_top():
            for desc in (False, True):
                got = _device(env, gpu, call_text("v", "Row(f=1)", limit=10, desc=desc))
                order = sorted(cur, key=lambda c: (-cur[c] if desc else cur[c], c))[:10]
                assert got.columns.tolist() == order and got.values.tolist() == [cur[c] for c in order]
            return set(_device(env, gpu, call_text("v", "Row(f=1)", limit=10)).columns.tolist())
        top = check_top()
        enters = next(int(c) for c in cols[::-1] if int(c) not in top)
        env.q("i", f"Set({enters}, v=-77777)")
        cur[enters] = -77777
        top = check_top()
        assert enters in top
        leaves = next(c for c in sorted(top) if c != enters)
        env.q("i", f"Set({leaves}, v=88888)")
        cur[leaves] = 88888
        assert leaves not in check_top()
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
        for field, filt, mask in (("m", "", np.ones(len(data.cols), bool)), ("v", "Row(f=1)", data.rows[1])):
            n0 = gpu.stats()["sortDevice"]
            r = ex.execute("i", call_text(field, filt, limit=300, desc=True)).results[0]
            assert gpu.stats()["sortDevice"] == n0 + 1
            check(r, window(oracle(data, field, mask, True), 0, 300))
            frags = holder.view("i", field, "bsig_" + field).all_fragments()
            assert frags and all(f.is_cold() for f in frags), "Sort read a BSI fragment on the host"
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
                        "tests/test_gpu_sort.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
