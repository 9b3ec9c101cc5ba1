"""TopK(field=, k=) on the device: row_filter_counts_kernel, the per-row
programs route and the host path against numpy, on the smallest shape that
takes every branch of the kernel: three shards with a gap, containers at keys
0, 7 and 15, 70 rows (more than a wave's lanes and a workgroup's waves), all
three container encodings among the rows and in the staged filter row, arrays
small enough for one lane and arrays for a whole wave, a row at one key only,
a row absent from a shard, a row that meets no filter, ties, sparse row ids up
to 2^40.  Every answer is an exact integer."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pilosa_amd import executor as executor_mod
from pilosa_amd.executor import Executor
from pilosa_amd.models.holder import Holder

from tests.helpers import SW, Env
from tests.topk_util import A_IDS, FILTERS, KS, SHARDS, Data, call_text, flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "PILOSA_TOPK_WIDTH_CHILD"
ROUTES = (("kernel", "topkDevice"), ("programs", "topkPrograms"))


@pytest.fixture(scope="module")
def envs():
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    env.data = Data()
    env.data.load(env)
    gpu = GpuExecutor(env.holder, "cuda:0", executor=env.executor)
    env.executor.gpu = gpu
    yield env, gpu
    env.close()


def _routes(ex, gpu, q, monkeypatch):
    """The request answered by the kernel route, by the programs route and by
    the host: each device route's counter rises by exactly one (the other
    stays), no device fault is recorded, the three answers are equal."""
    f0 = executor_mod.DEVICE_FAULTS[0]
    answers = []
    for route, counter in ROUTES:
        st0 = gpu.stats()
        with monkeypatch.context() as m:
            m.setenv("PILOSA_TOPK_DEVICE", route)
            answers.append(flat(ex.execute("i", q).results[0]))
        st1 = gpu.stats()
        for _, other in ROUTES:
            assert st1[other] == st0[other] + (1 if other == counter else 0), (route, other, q)
    st0 = gpu.stats()
    with monkeypatch.context() as m:
        m.setenv("PILOSA_TOPK_DEVICE", "0")
        answers.append(flat(ex.execute("i", q).results[0]))
    st1 = gpu.stats()
    assert (st1["topkDevice"], st1["topkPrograms"]) == (st0["topkDevice"], st0["topkPrograms"])
    assert executor_mod.DEVICE_FAULTS[0] == f0
    assert answers[0] == answers[1] == answers[2], q
    return answers[0]


def test_fixture_shape(envs):
    env, gpu = envs
    d = env.data

    def enc(field, row=None):
        v = gpu.view_arena("i", field, "standard", list(SHARDS))
        m = v.t_meta.cpu().numpy()
        if row is not None:
            rp = v.t_rowptr.cpu().numpy().reshape(v.S, v.D + 1).astype(np.int64)
            sb = v.t_shard_base.cpu().numpy()
            dd = v.dense(row)
            m = np.concatenate([m[sb[s] + rp[s, dd]:sb[s] + rp[s, dd + 1]] for s in range(v.S)])
        return m
    if SW >= 1 << 20:
        assert set(((enc("a") >> 4) & 3).tolist()) >= {1, 2, 3}          # 1 array, 2 bitmap, 3 run
        assert set(((enc("f", 1) >> 4) & 3).tolist()) >= {1, 2, 3}       # the staged filter row
        ma = enc("a")
        arr = (ma >> 6 & 0x1FFFF)[((ma >> 4) & 3) == 1]
        assert (arr <= 32).any() and (arr > 32).any() and (arr > 512).any()   # lane-owned and cooperative arrays
    if SW == 1 << 20:
        assert set(((d.cols % np.uint64(SW)) >> np.uint64(16)).tolist()) == {0, 7, 15}
        assert set(((d.cols[d.rows["a"][A_IDS[2]]] % np.uint64(SW)) >> np.uint64(16)).tolist()) == {7}
    v = gpu.view_arena("i", "a", "standard", list(SHARDS))
    assert v.D == 70 > 64 and int(v.rows[-1]) >= 1 << 40


@pytest.mark.parametrize("filt", FILTERS)
def test_routes_equal_numpy(envs, monkeypatch, filt):
    env, gpu = envs
    for field in ("a", "n"):
        for k in KS:
            want = env.data.expected(field, filt, k)
            assert _routes(env.executor, gpu, call_text(field, filt, k), monkeypatch) == want, (field, filt, k)


def test_default_route(envs, monkeypatch):
    """Without PILOSA_TOPK_DEVICE the route is TOPK_DEFAULT_ROUTE."""
    from pilosa_amd.ops import gpu_executor as ge
    env, gpu = envs
    monkeypatch.delenv("PILOSA_TOPK_DEVICE", raising=False)
    counter = dict(ROUTES)[ge.TOPK_DEFAULT_ROUTE]
    st0 = gpu.stats()
    assert flat(env.q1("i", call_text("a", "Row(f=1)", 5))) == env.data.expected("a", "Row(f=1)", 5)
    assert gpu.stats()[counter] == st0[counter] + 1


@pytest.mark.parametrize("rpb", ["0", "64", "1"])
def test_rows_per_workgroup(envs, monkeypatch, rpb):
    """One workgroup per (shard, key) for all 70 rows, chunks of 64 (a last
    chunk of 6) and one row per workgroup."""
    env, gpu = envs
    monkeypatch.setenv("PILOSA_TOPK_ROWS_PER_BLOCK", rpb)
    monkeypatch.setenv("PILOSA_TOPK_DEVICE", "kernel")
    for filt in ("Row(f=1)", "Not(Row(f=1))"):
        assert flat(env.q1("i", call_text("a", filt))) == env.data.expected("a", filt)


@pytest.mark.parametrize("rpw", ["16", "32", "64"])
def test_rows_per_wave_step(envs, monkeypatch, rpw):
    """70 rows looked up 16, 32 and 64 per wave and step: several steps per
    wave, a last step that is not full, waves without a row."""
    env, gpu = envs
    monkeypatch.setenv("PILOSA_TOPK_ROWS_PER_WAVE", rpw)
    monkeypatch.setenv("PILOSA_TOPK_DEVICE", "kernel")
    for filt in ("Row(f=1)", "Intersect(Row(f=1), Row(g=1))"):
        assert flat(env.q1("i", call_text("a", filt))) == env.data.expected("a", filt)


def test_without_keymask(envs, monkeypatch):
    """A view without the key-presence table: the meta walk finds the containers."""
    env, gpu = envs
    v = gpu.view_arena("i", "a", "standard", list(SHARDS))
    monkeypatch.setenv("PILOSA_KEYMASK", "0")
    monkeypatch.setenv("PILOSA_TOPK_DEVICE", "kernel")
    saved = getattr(v, "_keymask", None)
    v._keymask = None
    try:
        assert int(v.viewdev()["keymask"]) == 0
        for filt in ("Row(f=1)", "Row(w > 500)"):
            assert flat(env.q1("i", call_text("a", filt))) == env.data.expected("a", filt)
    finally:
        v._keymask = saved


def test_options_shards(envs, monkeypatch):
    env, gpu = envs
    q = f"Options({call_text('a', 'Row(f=1)', 9)}, shards=[1, 3])"
    assert _routes(env.executor, gpu, q, monkeypatch) == env.data.expected("a", "Row(f=1)", 9, shards=[1, 3])


def test_after_writes(monkeypatch):
    """A Set that creates a new row and a Clear that breaks a tie reach the
    resident arena before the next TopK."""
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env(gpu=lambda h: GpuExecutor(h, "cuda:0"))
    try:
        gpu = env.executor.gpu
        gpu.executor = env.executor
        env.create_index("i")
        env.field("i", "a")
        env.field("i", "f")
        rng = np.random.default_rng(4)
        cols = np.concatenate([s * SW + rng.choice(SW // 2, 3000, replace=False) for s in SHARDS]).astype(np.uint64)
        member = {r: set(cols[rng.random(len(cols)) < p].tolist()) for r, p in ((1, 0.5), (2, 0.1), (5, 0.02))}
        member[3] = set(member[2])                              # a tie: 2 before 3
        in_f = set(cols[rng.random(len(cols)) < 0.5].tolist())
        idx = env.holder.index("i")
        for r, cc in member.items():
            idx.field("a").import_bits(np.full(len(cc), r, np.uint64), np.fromiter(cc, np.uint64))
        idx.field("f").import_bits(np.ones(len(in_f), np.uint64), np.fromiter(in_f, np.uint64))

        def want(filt):
            out = [(r, len(cc & in_f) if filt else len(cc)) for r, cc in member.items()]
            return sorted((p for p in out if p[1]), key=lambda p: (-p[1], p[0]))
        for filt in ("", "Row(f=1)"):
            got = _routes(env.executor, gpu, call_text("a", filt), monkeypatch)
            assert got == want(filt) and [r for r, _ in got][1:3] == [2, 3]
        st0 = gpu.stats()
        new_col = 3 * SW + SW // 2 + 1
        gone = next(c for c in sorted(member[2]) if c in in_f)
        env.q("i", f"Set({new_col}, a=77) Set({new_col}, f=1) Clear({gone}, a=2)")
        member[77] = {new_col}
        member[2] = member[2] - {gone}
        in_f.add(new_col)
        for filt in ("", "Row(f=1)"):
            got = _routes(env.executor, gpu, call_text("a", filt), monkeypatch)
            assert got == want(filt) and [r for r, _ in got][1:3] == [3, 2] and got[-1] == (77, 1)
        st1 = gpu.stats()
        assert st1["rebuilds"] == st0["rebuilds"] and st1["shardUpdates"] > st0["shardUpdates"]
    finally:
        env.close()


def test_lazily_opened_holder_stays_cold(monkeypatch):
    import shutil
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    data = Data()
    data.load(env)
    env.holder.close()
    holder = Holder(env.dir, lazy_fragments=True).open()
    gpu = GpuExecutor(holder, "cuda:0")
    ex = Executor(holder, gpu=gpu)
    gpu.executor = ex
    try:
        for route, counter in ROUTES:
            for field, filt in (("a", ""), ("a", "Row(f=1)"), ("n", "Intersect(Row(f=1), Row(g=1))")):
                st0, f0 = gpu.stats(), executor_mod.DEVICE_FAULTS[0]
                with monkeypatch.context() as m:
                    m.setenv("PILOSA_TOPK_DEVICE", route)
                    got = flat(ex.execute("i", call_text(field, filt)).results[0])
                assert gpu.stats()[counter] == st0[counter] + 1 and executor_mod.DEVICE_FAULTS[0] == f0
                assert got == data.expected(field, filt)
                frags = holder.view("i", field, "standard").all_fragments()
                assert frags and all(f.is_cold() for f in frags), "TopK read a fragment on the host"
        # the host path, last (it warms the fragments)
        assert _routes(ex, gpu, call_text("a", "Row(f=1)", 5), monkeypatch) == data.expected("a", "Row(f=1)", 5)
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
                        "tests/test_gpu_topk.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
