"""ConstRow(columns=[...]) on the device (const_row_kernel, K30): the dense view
read back against numpy, and every consumer against the host path, on the
smallest shapes at which the kernel can go wrong -- the fixture of
tests/test_gpu_extract.py (three shards with a gap) and one column list per
boundary: the bits on both sides of a 32- and a 64-bit word, of a container
key and of a shard; keys 0, 7 and 15 only; a requested shard without a
column; a unit of one column; a unit of 5,000 columns (more than a wave's
lanes, several per word); a full container; duplicates; and a list that lies
outside the shards altogether.  Every answer is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pilosa_amd import shardwidth
from pilosa_amd.executor import Executor
from pilosa_amd.models.holder import Holder

from tests.const_row_util import meta_oracle, random_tree, row_of, text, view_oracle
from tests.distinct_util import load
from tests.helpers import SW, Env, cols
from tests.test_gpu_extract import SHARDS, Data
from tests.test_mesh import _canon

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "PILOSA_CONSTROW_WIDTH_CHILD"
U = SW // 16                      # columns per sixteenth of a shard (one container key at 2^20)
UNIT = min(SW, 65536)             # columns of one device unit
DSHARDS = shardwidth.device_shards(SHARDS)


def _unit_base(shard, key):
    """First column of the device unit that holds sixteenth ``key`` of ``shard``."""
    return (shard * SW + key * U) // UNIT * UNIT


def _lists():
    rng = np.random.default_rng(41)
    s0, s1, s3 = (s * SW for s in SHARDS)
    out = {
        "word": [s0 + x for x in (0, 31, 32, 63, 64)] + [s3 + 7 * U + x for x in (31, 32, 63, 64, 65)],
        "key": [s1 + UNIT - 1, s1 + UNIT, s0 + UNIT - 1, s3 + UNIT],       # (past a 2^16 shard: not requested)
        "shard": [s0 + SW - 1, s1, s1 + SW - 1, s3, s3 + SW - 1, (1 << 20) - 1, 1 << 20],
        "keys 0 7 15": [s * SW + k * U + x for s in SHARDS for k in (0, 7, 15) for x in (0, 5, U - 1)],
        "empty shard": [s0 + 3, s0 + 9 * U + 1, s3 + 100, s3 + 15 * U + 4],  # nothing in shard 1
        "one column": [s3 + 7 * U + 123],
        "5000 in a unit": (_unit_base(SHARDS[1], 7) + np.sort(rng.choice(UNIT, 5000, replace=False))).tolist(),
        "full container": (_unit_base(SHARDS[2], 15) + np.arange(UNIT)).tolist(),   # the last unit of the last shard
        "duplicates": [s1 + 40, s0 + 7, s1 + 40, s1 + 40, s0 + 7, s3 + SW - 1, s3 + SW - 1, s1 + 41],
    }
    out["mixed"] = out["word"] + out["key"] + out["shard"] + out["keys 0 7 15"] + out["duplicates"] + \
        [2 * SW + 5, 5 * SW + 1]                                               # + an absent and an unrequested shard
    return out


LISTS = _lists()
OUTSIDE = [2 * SW + 1, 2 * SW + SW - 1, 4 * SW, 77 * SW + 3]
SMALL = [k for k in LISTS if k not in ("5000 in a unit", "full container")]


@pytest.fixture(scope="module")
def envs():
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    env.data = d = Data()
    load(env, d)
    env.field("i", "mx", type="mutex")
    rng = np.random.default_rng(5)
    has = rng.random(len(d.cols)) < 0.6
    env.holder.index("i").field("mx").import_bits(rng.integers(0, 5, int(has.sum())).astype(np.uint64), d.cols[has])
    gpu = GpuExecutor(env.holder, "cuda:0", executor=env.executor)
    env.executor.gpu = gpu
    env.executor.strict_gpu = True        # a device error is an error, not a silent host answer
    # columns that hold values, spread over every key the fixture fills
    env.real = d.cols[::5].tolist()
    yield env, gpu
    env.close()


def _host(env, gpu, monkeypatch, q):
    """The same request with the planner declining: the host path."""
    def decline(*a, **k):
        raise NotImplementedError
    with monkeypatch.context() as m:
        m.setattr(gpu, "plan", decline)
        n0 = gpu.stats()["constRowDevice"]
        r = env.q1("i", q)
        assert gpu.stats()["constRowDevice"] == n0
    return r


def _device(env, gpu, q, views=None):
    n0 = gpu.stats()["constRowDevice"]
    r = env.q1("i", q)
    moved = gpu.stats()["constRowDevice"] - n0
    assert moved >= 1 if views is None else moved == views, f"{moved} views built: {q[:60]}"
    return r


# ---------------------------------------------------------------- the view itself
@pytest.mark.parametrize("name", list(LISTS))
def test_view_read_back_matches_numpy(envs, name):
    env, gpu = envs
    listed = LISTS[name]
    from pilosa_amd.executor import const_row_columns
    from pilosa_amd.pql import Call
    rv = gpu.engine.const_row_view(const_row_columns(Call("ConstRow", {"columns": list(listed)})), DSHARDS)
    assert rv is not None and rv.S == len(DSHARDS) and rv.D == 1 and list(rv.shards) == list(DSHARDS)
    words, cards = view_oracle(listed, DSHARDS, shardwidth.ARENA_WIDTH)
    got = rv.t_payload.cpu().numpy().view(np.uint32).reshape(rv.S * 16, 2048)
    bad = np.flatnonzero((got != words).any(axis=1))
    assert not len(bad), f"units {bad[:8].tolist()} differ"
    assert rv.t_meta.cpu().numpy().tolist() == meta_oracle(cards).tolist()
    assert int(cards.sum()) == len(row_of(listed, SHARDS))
    if name == "full container":
        assert int(cards.max()) == 65536 and (SW != 1 << 20 or int(cards[-1]) == 65536)   # meta_n's 17th bit
    if name == "empty shard":
        per = cards.reshape(len(DSHARDS), 16).sum(axis=1)
        assert (per == 0).any() and not (got.reshape(len(DSHARDS), -1)[per == 0]).any()
    if name == "one column":
        assert sorted(cards.tolist())[-2:] == [0, 1]


def test_a_list_outside_the_shards_is_empty_without_a_launch(envs):
    env, gpu = envs
    from pilosa_amd.ops.gpu_executor import EMPTY
    from pilosa_amd.pql import parse_string
    assert gpu.engine.const_row_view(np.array(OUTSIDE, np.uint64), DSHARDS) is None
    env.q1("i", "Count(Row(f=1))")
    s0 = gpu.stats()
    assert gpu.plan("i", parse_string(text(OUTSIDE)).calls[0], list(SHARDS)) is EMPTY
    assert env.q1("i", f"Count({text(OUTSIDE)})") == 0
    assert cols(env.q1("i", text(OUTSIDE))) == []
    assert env.q1("i", f"Count(Union({text(OUTSIDE)}, {text(OUTSIDE[:2])}))") == 0
    s1 = gpu.stats()
    assert s1["constRowDevice"] == s0["constRowDevice"] and s1["launches"] == s0["launches"]
    # next to a row it is the row alone: one count launch, no view
    assert env.q1("i", f"Count(Union(Row(f=1), {text(OUTSIDE)}))") == env.q1("i", "Count(Row(f=1))")
    assert gpu.stats()["constRowDevice"] == s0["constRowDevice"]


# ---------------------------------------------------------------- consumers
SHAPES = ["{}", "Count({})", "Count(Intersect(Row(f=1), {}))", "Intersect(Row(f=1), {})", "Difference(Row(f=1), {})",
          "Difference({}, Row(f=1))", "Union(Row(f=6), {})", "Xor(Row(f=1), {})", "Not({})", "Count(Not({}))",
          "Shift({}, n=1)", "Count(Shift({}, n=1))", "Shift({}, n=65)",
          "Sum({}, field=v)", "Min({}, field=m)", "Max({}, field=w)", "TopK({}, field=f)", "TopK({}, field=f, k=2)",
          "Distinct({}, field=v)", "Percentile({}, field=v, nth=50)", "Sort({}, field=v, limit=50)",
          "Sort({}, field=d32, sort-desc=true)",
          "Extract({}, Rows(field=v), Rows(field=f), Rows(field=mx))", "Extract({}, Rows(field=m), limit=40, offset=3)",
          "GroupBy(Rows(field=f), filter={})", "GroupBy(Rows(field=f), filter={}, aggregate=Sum(field=v))"]


@pytest.mark.parametrize("name", SMALL)
def test_consumers_equal_the_host_path(envs, monkeypatch, name):
    """The boundary list next to columns that hold values, through every consumer."""
    env, gpu = envs
    t = text(LISTS[name] + env.real)
    for shape in SHAPES:
        q = shape.format(t)
        got = _device(env, gpu, q)
        assert _canon([got]) == _canon([_host(env, gpu, monkeypatch, q)]), (name, shape)
    want = row_of(LISTS[name] + env.real, SHARDS)
    assert cols(env.q1("i", t)) == want and env.q1("i", f"Count({t})") == len(want)


@pytest.mark.parametrize("name", ["5000 in a unit", "full container"])
def test_large_units_through_consumers(envs, monkeypatch, name):
    env, gpu = envs
    d = env.data
    t = text(LISTS[name] + env.real)
    want = row_of(LISTS[name] + env.real, SHARDS)
    assert env.q1("i", f"Count({t})") == len(want) and len(want) >= 5000
    assert cols(_device(env, gpu, t)) == want
    f1 = set(d.cols[d.rows[1]].tolist()) | set(d.extra.tolist())
    assert _device(env, gpu, f"Count(Intersect(Row(f=1), {t}))") == len(f1 & set(want))
    for shape in ("Count(Difference(Row(f=1), {}))", "Count(Difference({}, Row(f=1)))", "Count(Not({}))",
                  "Count(Shift({}, n=1))", "Sum({}, field=v)", "TopK({}, field=f)", "Distinct({}, field=v)",
                  "Percentile({}, field=v, nth=50)", "Sort({}, field=v, limit=20)",
                  "Extract({}, Rows(field=v), Rows(field=f), Rows(field=mx), limit=300, offset=4000)",
                  "GroupBy(Rows(field=f), filter={})", "GroupBy(Rows(field=f), filter={}, aggregate=Sum(field=v))"):
        q = shape.format(t)
        assert _canon([_device(env, gpu, q)]) == _canon([_host(env, gpu, monkeypatch, q)]), shape


def test_shift_across_a_key_and_a_shard_boundary(envs, monkeypatch):
    env, gpu = envs
    s0, s1, s3 = (s * SW for s in SHARDS)
    listed = [s0 + UNIT - 1, s0 + SW - 1, s1 + SW - 1, s3 + SW - 1, s3 + 5, s1 + 63]
    got = cols(_device(env, gpu, f"Shift({text(listed)}, n=1)"))
    assert got == cols(_host(env, gpu, monkeypatch, f"Shift({text(listed)}, n=1)"))
    assert s0 + UNIT in got and s1 in got and s1 + 64 in got and s3 + 6 in got
    probe = [s0 + UNIT, s1, s3 + 7, s3 + 6]
    q = f"Count(Intersect(Shift({text(listed)}, n=1), {text(probe)}))"
    # (evaluation is per shard: a bit carried into the next shard meets that shard's bits only in a top-level row)
    assert _device(env, gpu, q, views=2) == _host(env, gpu, monkeypatch, q) == (2 if SW > UNIT else 1)


def test_counters_and_launches(envs):
    env, gpu = envs
    t = text(LISTS["mixed"])
    env.q1("i", f"Count(Intersect(Row(f=1), {t}))")          # the arenas are resident from here on
    for q, views, launches in ((f"Count({t})", 1, 2),                             # K30 + the count
                               (t, 1, 2),                                         # K30 + the materialisation
                               (f"Count(Intersect(Row(f=1), {t}))", 1, 2),
                               (f"Count(Xor({t}, {text(LISTS['word'])}))", 2, 3)):
        s0 = gpu.stats()
        _device(env, gpu, q, views=views)
        assert gpu.stats()["launches"] == s0["launches"] + launches, q[:40]
    # views are not cached: the same list again builds again
    _device(env, gpu, f"Count({t})", views=1)


def test_device_knob_off_sends_the_call_to_the_host(envs, monkeypatch):
    env, gpu = envs
    t = text(LISTS["mixed"] + env.real)
    want = {q: env.q1("i", q) for q in (f"Count({t})", f"Sum({t}, field=v)", f"Count(Intersect(Row(f=1), {t}))")}
    monkeypatch.setenv("PILOSA_CONSTROW_DEVICE", "0")
    n0 = gpu.stats()["constRowDevice"]
    for q, w in want.items():
        assert env.q1("i", q) == w
    assert cols(env.q1("i", t)) == row_of(LISTS["mixed"] + env.real, SHARDS)
    assert gpu.stats()["constRowDevice"] == n0
    monkeypatch.delenv("PILOSA_CONSTROW_DEVICE")
    _device(env, gpu, f"Count({t})", views=1)


def test_a_count_request_holding_a_const_row_falls_back_to_the_planner(envs):
    """Five Count calls that would take the native batch path; one holds a ConstRow."""
    env, gpu = envs
    d = env.data
    t = text(LISTS["mixed"] + env.real)
    qs = ["Count(Row(f=1))", "Count(Intersect(Row(f=1), Row(f=4)))", f"Count(Intersect(Row(f=1), {t}))",
          "Count(Union(Row(f=2), Row(f=3)))", "Count(Row(f=6))"]
    n0 = gpu.stats()["constRowDevice"]
    got = env.q("i", " ".join(qs))
    assert gpu.stats()["constRowDevice"] == n0 + 1
    assert got == [env.q1("i", q) for q in qs]
    f1 = set(d.cols[d.rows[1]].tolist()) | set(d.extra.tolist())
    assert got[2] == len(f1 & set(row_of(LISTS["mixed"] + env.real, SHARDS))) and got[4] == 1


def test_forty_random_trees_equal_the_host_path(envs, monkeypatch):
    env, gpu = envs
    rng = np.random.default_rng(8)
    lists = [LISTS[k] + env.real[i::3] for i, k in enumerate(("word", "key", "shard"))] + \
        [LISTS["keys 0 7 15"], LISTS["duplicates"], OUTSIDE, env.real]
    rows = ["Row(f=1)", "Row(f=4)", "Row(f=6)", "Row(f=9)", "Row(v > 100)"]
    n0 = gpu.stats()["constRowDevice"]
    for i in range(40):
        q = random_tree(rng, lists, rows)
        q = q if i % 2 else f"Count({q})"
        assert _canon([env.q1("i", q)]) == _canon([_host(env, gpu, monkeypatch, q)]), q[:200]
    assert gpu.stats()["constRowDevice"] >= n0 + 20


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
    ex.strict_gpu = True
    gpu.executor = ex
    try:
        listed = data.cols[::3]
        mask = np.zeros(len(data.cols), bool)
        mask[::3] = True
        n0 = gpu.stats()["constRowDevice"]
        r = ex.execute("i", f"Sum({text(listed.tolist())}, field=v)").results[0]
        assert gpu.stats()["constRowDevice"] == n0 + 1
        assert (r.val, r.count) == (int(data.vals["v"][mask & data.has["v"]].sum()), int((mask & data.has["v"]).sum()))
        frags = holder.view("i", "v", "bsig_v").all_fragments()
        assert frags and all(f.is_cold() for f in frags), "a ConstRow filter read a BSI fragment on the host"
    finally:
        ex.close()
        holder.close()
        env.executor.close()
        shutil.rmtree(env.dir, ignore_errors=True)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("exp", [16, 22])
def test_shard_widths(exp):
    """This file again in a fresh interpreter at another shard width (the
    width is fixed per process): at 2^16 a shard is one device unit and only
    key 0 is written; at 2^22 a shard is four device shards."""
    if os.environ.get(CHILD):
        return   # the child runs every other test of the file, never this one again
    env = dict(os.environ, PILOSA_SHARD_WIDTH=str(exp))
    env[CHILD] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "--timeout", "300", "--timeout-method", "thread", "-k", "not test_shard_widths",
                        "tests/test_gpu_const_row.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
