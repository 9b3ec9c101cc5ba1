"""GroupBy(..., aggregate=Sum(field=)) on the device (bsi_group_sum_kernel)
against numpy and against the host executor, on the smallest shape that takes
every branch of the kernel: three shards with a gap, containers at keys 0, 7
and 15, all three container encodings in the planes and in the group rows,
nine rows in the first field (more than the four waves of a workgroup), a row
that lives at one key only, a group without any value, a non-zero base and a
depth-40 field that needs several plane slabs.  Every answer is an exact
integer."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pilosa_amd import executor as executor_mod
from pilosa_amd.executor import Executor
from pilosa_amd.models.holder import Holder

from tests.groupby_sum_util import SHARDS, Data, call_text, flat
from tests.helpers import SW, Env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "PILOSA_GROUPSUM_WIDTH_CHILD"
FILTERS = ["", "Row(f=1)", "Intersect(Row(f=1), Row(g=1))", "Not(Row(f=1))", "Row(w > 500)"]
FIELDS = {1: ["a"], 2: ["a", "b"], 3: ["a", "b", "c"]}


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


def _device(ex, gpu, q, monkeypatch):
    """The request answered by bsi_group_sum_kernel (every group count routed
    to it), then by the host path (PILOSA_GROUPSUM_DEVICE=0): the counter
    rises once and then stays, no device fault is recorded, the two answers
    are equal."""
    st0, f0 = gpu.stats(), executor_mod.DEVICE_FAULTS[0]
    with monkeypatch.context() as m:
        m.setenv("PILOSA_GROUPSUM_MIN_GROUPS", "1")
        got = flat(ex.execute("i", q).results[0])
    st1 = gpu.stats()
    assert st1["groupSumDevice"] == st0["groupSumDevice"] + 1, "bsi_group_sum_kernel did not answer"
    assert st1["launches"] > st0["launches"]
    with monkeypatch.context() as m:
        m.setenv("PILOSA_GROUPSUM_DEVICE", "0")
        host = flat(ex.execute("i", q).results[0])
    assert gpu.stats()["groupSumDevice"] == st1["groupSumDevice"]
    assert executor_mod.DEVICE_FAULTS[0] == f0
    assert got == host, q
    return got


def test_fixture_shape(envs):
    env, gpu = envs
    d = env.data

    def enc(field, view):
        m = gpu.view_arena("i", field, view, list(SHARDS)).t_meta
        m = m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)
        return set(((m >> 4) & 3).tolist())
    assert enc("big", "bsig_big") >= {1, 2, 3}      # 1 array, 2 bitmap, 3 run
    if SW >= 1 << 20:
        assert enc("v", "bsig_v") >= {1, 2, 3} and enc("a", "standard") >= {1, 2, 3}
    if SW == 1 << 20:
        keys = set(((d.cols % np.uint64(SW)) >> np.uint64(16)).tolist())
        assert keys == {0, 3, 7, 15}                # 3: the columns without any value
        assert set(((d.cols[d.rows["a"][3]] % np.uint64(SW)) >> np.uint64(16)).tolist()) == {7}
    depth = {n: env.holder.field("i", n).bsi_group(n).bit_depth for n in ("v", "w", "big")}
    assert depth["big"] == 40 and depth["v"] == 11 and env.holder.field("i", "w").bsi_group("w").base == 100
    assert depth["big"] > gpu.engine.GROUPSUM_SLAB      # several slabs at the default
    assert int(np.abs(d.vals["big"]).max()) > 1 << 38
    assert [x for x in d.expected(["a"], "w") if x[1] > 0 and x[3] == 0]   # count > 0, no value


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_device_equals_numpy_and_host(envs, monkeypatch, k, filt):
    env, gpu = envs
    for vf in ("v", "w", "big"):
        want = env.data.expected(FIELDS[k], vf, filt)
        assert len(want) >= (8 if k == 1 else 30)
        assert _device(env.executor, gpu, call_text(FIELDS[k], vf, filt), monkeypatch) == want, (k, vf, filt)


def test_same_groups_without_aggregate(envs, monkeypatch):
    env, gpu = envs
    for k in (1, 2, 3):
        n0 = gpu.stats()["groupSumDevice"]
        plain = flat(env.q1("i", call_text(FIELDS[k], None, "Row(f=1)")))
        assert gpu.stats()["groupSumDevice"] == n0
        assert plain == env.data.expected(FIELDS[k], None, "Row(f=1)")
        agg = _device(env.executor, gpu, call_text(FIELDS[k], "v", "Row(f=1)"), monkeypatch)
        assert [(g[0], g[1]) for g in agg] == [(g[0], g[1]) for g in plain]


@pytest.mark.parametrize("kw", [{"limit": 7}, {"previous": [2, 3]}, {"previous": [4, 1], "limit": 5},
                                {"limit": 11, "offset": 3}])
def test_paging(envs, monkeypatch, kw):
    env, gpu = envs
    for filt in ("", "Row(f=1)"):
        want = env.data.expected(["a", "b"], "w", filt, **kw)
        assert want
        assert _device(env.executor, gpu, call_text(["a", "b"], "w", filt, **kw), monkeypatch) == want


def test_matrix_route(envs, monkeypatch):
    """The two-field count matrix yields the groups; the sums follow in one
    pass over the final list."""
    from pilosa_amd.ops import gpu_executor as ge
    from pilosa_amd.ops import groupby
    env, gpu = envs
    calls = []
    real = groupby.pair_count_matrix
    monkeypatch.setattr(groupby, "pair_count_matrix", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(ge, "GROUPBY_MATRIX_MIN", 1)
    for filt, kw in (("", {}), ("Row(f=1)", {}), ("Row(f=1)", {"limit": 6}), ("", {"previous": [3, 2]})):
        n = len(calls)
        want = env.data.expected(["a", "b"], "big", filt, **kw)
        assert _device(env.executor, gpu, call_text(["a", "b"], "big", filt, **kw), monkeypatch) == want
        assert len(calls) == n + 1, "the count matrix was not used"


@pytest.mark.parametrize("slab", ["1", "4"])
def test_slab_sizes(envs, monkeypatch, slab):
    """Depth 11 in slabs of 1 and of 4 planes (a last slab of 3): slab
    boundaries, the count taken once, a last slab that is not full."""
    env, gpu = envs
    for k, filt in ((1, ""), (2, "Row(f=1)"), (3, "Not(Row(f=1))")):
        q = call_text(FIELDS[k], "v", filt)
        default = _device(env.executor, gpu, q, monkeypatch)
        with monkeypatch.context() as m:
            m.setenv("PILOSA_GROUPSUM_SLAB", slab)
            assert _device(env.executor, gpu, q, m) == default == env.data.expected(FIELDS[k], "v", filt)


def test_group_chunks(envs, monkeypatch):
    """Launches of at most 4 groups, and workgroups of 3 groups (fewer than
    the waves of a workgroup)."""
    from pilosa_amd.ops import gpu_executor as ge
    env, gpu = envs
    want = env.data.expected(["a", "b"], "w", "Row(f=1)")
    q = call_text(["a", "b"], "w", "Row(f=1)")
    with monkeypatch.context() as m:
        m.setattr(ge, "MAX_GROUPS_PER_LAUNCH", 4)
        l0 = gpu.stats()["launches"]
        assert _device(env.executor, gpu, q, m) == want
        assert gpu.stats()["launches"] - l0 >= len(want) // 4
    with monkeypatch.context() as m:
        m.setenv("PILOSA_GROUPSUM_CHUNK", "3")
        assert _device(env.executor, gpu, q, m) == want
    assert _device(env.executor, gpu, call_text(["a"], "w"), monkeypatch) == env.data.expected(["a"], "w")


def test_default_route_is_the_per_filter_kernel(envs, monkeypatch):
    """No group count is known at which bsi_group_sum_kernel is the faster
    one (profiles/groupby_sum/README.md): without the override the same
    programs go through the per-filter kernel, with equal answers."""
    from pilosa_amd.ops import gpu_executor as ge
    env, gpu = envs
    monkeypatch.delenv("PILOSA_GROUPSUM_MIN_GROUPS", raising=False)
    assert ge.GROUPSUM_MIN_GROUPS is None
    for k, vf, filt in ((1, "w", ""), (2, "big", "Row(f=1)"), (3, "v", "Not(Row(f=1))")):
        st0, f0 = gpu.stats(), executor_mod.DEVICE_FAULTS[0]
        got = flat(env.q1("i", call_text(FIELDS[k], vf, filt)))
        st1 = gpu.stats()
        assert st1["groupSumPerFilter"] == st0["groupSumPerFilter"] + 1
        assert st1["groupSumDevice"] == st0["groupSumDevice"] and executor_mod.DEVICE_FAULTS[0] == f0
        assert got == env.data.expected(FIELDS[k], vf, filt)
    with monkeypatch.context() as m:       # the threshold: 9 groups stay, 45 take the kernel
        m.setenv("PILOSA_GROUPSUM_MIN_GROUPS", "10")
        st0 = gpu.stats()
        assert flat(env.q1("i", call_text(["a"], "v"))) == env.data.expected(["a"], "v")
        assert flat(env.q1("i", call_text(["a", "b"], "v"))) == env.data.expected(["a", "b"], "v")
        st1 = gpu.stats()
        assert (st1["groupSumPerFilter"] - st0["groupSumPerFilter"],
                st1["groupSumDevice"] - st0["groupSumDevice"]) == (1, 1)


def test_options_shards(envs, monkeypatch):
    env, gpu = envs
    q = f"Options({call_text(['a', 'b'], 'v', 'Row(f=1)')}, shards=[1, 3])"
    assert _device(env.executor, gpu, q, monkeypatch) == env.data.expected(["a", "b"], "v", "Row(f=1)", shards=[1, 3])


def test_after_writes(monkeypatch):
    """Writes to the group field and to the int field through the executor
    reach the resident arenas (patched in place, never rebuilt) before the
    next GroupBy."""
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env(gpu=lambda h: GpuExecutor(h, "cuda:0"))
    try:
        gpu = env.executor.gpu
        gpu.executor = env.executor
        env.create_index("i")
        env.field("i", "a")
        env.field("i", "v", type="int", min=-1000, max=1000)
        rng = np.random.default_rng(4)
        cols = np.concatenate([s * SW + rng.choice(SW // 2, 3000, replace=False) for s in SHARDS])
        vals = rng.integers(-900, 901, len(cols))
        arow = rng.integers(1, 4, len(cols))
        idx = env.holder.index("i")
        idx.field("v").import_values(cols.astype(np.uint64), vals)
        idx.field("a").import_bits(arow.astype(np.uint64), cols.astype(np.uint64))
        val = dict(zip(cols.tolist(), vals.tolist()))
        member = {(int(r), int(c)) for r, c in zip(arow, cols)}

        def want():
            out = []
            for r in sorted({r for r, _ in member}):
                cs = [c for rr, c in member if rr == r]
                have = [val[c] for c in cs if c in val]
                out.append(((r,), len(cs), sum(have), len(have)))
            return out
        q = "GroupBy(Rows(a), aggregate=Sum(field=v))"
        assert _device(env.executor, gpu, q, monkeypatch) == want()
        st0 = gpu.stats()
        new_col, moved, cleared = 3 * SW + SW // 2 + 1, int(cols[0]), int(cols[1])
        env.q("i", f"Set({new_col}, a=7) Set({new_col}, v=1000) Set({moved}, a=2) Set({moved}, v=-1000) "
                   f"Clear({cleared}, v={val[cleared]})")
        member |= {(7, new_col), (2, moved)}
        val[new_col], val[moved] = 1000, -1000
        del val[cleared]
        got = _device(env.executor, gpu, q, monkeypatch)
        assert got == want() and got[-1] == ((7,), 1, 1000, 1)
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
        for k, vf, filt in ((2, "big", ""), (3, "v", "Row(f=1)")):
            st0, f0 = gpu.stats(), executor_mod.DEVICE_FAULTS[0]
            with monkeypatch.context() as m:
                m.setenv("PILOSA_GROUPSUM_MIN_GROUPS", "1")
                got = flat(ex.execute("i", call_text(FIELDS[k], vf, filt)).results[0])
            assert gpu.stats()["groupSumDevice"] == st0["groupSumDevice"] + 1
            assert executor_mod.DEVICE_FAULTS[0] == f0
            assert got == data.expected(FIELDS[k], vf, filt)
            frags = holder.view("i", vf, "bsig_" + vf).all_fragments()
            assert frags and all(f.is_cold() for f in frags), "GroupBy read a BSI fragment on the host"
        # the host path, last (it warms the fragments): equal answers, counter unchanged
        assert _device(ex, gpu, call_text(FIELDS[2], "big"), monkeypatch) == data.expected(FIELDS[2], "big")
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
                        "tests/test_gpu_groupby_sum.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
