"""Percentile(field=, nth=): exact nearest-rank selection over BSI int fields,
on the host path.  The reference has no such call, so every answer is pinned
to a sort of the known values (numpy); all answers are exact integers."""
import json
import shutil
import tempfile
import time
import urllib.request

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import ValCount
from pilosa_amd.ops.bsi import kth_plan, kth_replay

from tests.helpers import SW, Env
from tests.percentile_util import NTHS, boundary_nths, call_text, nth_for_rank, oracle, rank

SHARDS = (0, 1, 3)   # shard 2 is absent


class Data:
    """~2,000 columns with a value in v (min -1000, max 1000, base 0) drawn
    from 40 distinct values, most of them also in w (min 100, max 1100, base
    100), set field f: row 1 a random half, row 2 the negatives of v, row 3
    its non-negatives, row 5 exactly one column, row 9 nothing; f also holds
    columns without a value."""

    def __init__(self, n=2000, seed=11):
        rng = np.random.default_rng(seed)
        per = n // len(SHARDS)
        cols = np.concatenate([s * SW + rng.choice(SW, per + (1 if i < n - per * len(SHARDS) else 0), replace=False)
                               for i, s in enumerate(SHARDS)]).astype(np.uint64)
        distinct = np.unique(np.concatenate([[-1000, -1, 0, 1, 1000], rng.integers(-1000, 1001, 35)]))
        self.v_cols = cols
        self.v_vals = rng.choice(distinct, len(cols)).astype(np.int64)
        keep = rng.random(len(cols)) < 0.75
        self.w_cols = cols[keep]
        self.w_vals = rng.choice(np.unique(rng.integers(100, 1101, 40)), int(keep.sum())).astype(np.int64)
        novalue = np.array([5, SW + 5, 3 * SW + 5], np.uint64)   # in f, in neither int field
        assert not np.isin(novalue, cols).any()
        self.rows = {
            1: np.concatenate([cols[rng.random(len(cols)) < 0.5], novalue]),
            2: cols[self.v_vals < 0],
            3: np.concatenate([cols[self.v_vals >= 0], novalue[:1]]),
            5: cols[len(cols) // 2:len(cols) // 2 + 1],
            9: np.zeros(0, np.uint64),
        }

    def considered(self, field, row=None, shards=None):
        cols, vals = (self.v_cols, self.v_vals) if field == "v" else (self.w_cols, self.w_vals)
        m = np.ones(len(cols), bool)
        if row is not None:
            m &= np.isin(cols, self.rows[row])
        if shards is not None:
            m &= np.isin(cols // np.uint64(SW), np.asarray(shards, np.uint64))
        return vals[m]

    def load(self, env):
        env.create_index("i")
        env.field("i", "f")
        env.field("i", "v", type="int", min=-1000, max=1000)
        env.field("i", "w", type="int", min=100, max=1100, base=100)
        idx = env.holder.index("i")
        assert idx.field("w").bsi_group("w").base == 100 and idx.field("v").bsi_group("v").base == 0
        idx.field("v").import_values(self.v_cols, self.v_vals)
        idx.field("w").import_values(self.w_cols, self.w_vals)
        for r, c in self.rows.items():
            if len(c):
                idx.field("f").import_bits(np.full(len(c), r, np.uint64), c)


def cases(data):
    """(field, filter row or None, nth literal)."""
    out = []
    for field in ("v", "w"):
        for row in (None, 1):
            out += [(field, row, nth) for nth in NTHS]
            out += [(field, row, nth) for nth in boundary_nths(data.considered(field, row))]
    for row in (2, 3, 5, 9):    # all negative, all non-negative, one column, nothing
        out += [("v", row, nth) for nth in ("0", "0.1", "50", "99.9", "100")]
    return out


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data()
    e.data.load(e)
    yield e
    e.close()


def _filt(row):
    return f"Row(f={row})" if row is not None else ""


def test_host_path_matches_numpy(env):
    d = env.data
    assert len(d.considered("v")) == 2000 and 30 <= len(np.unique(d.v_vals)) <= 40
    assert sorted(set((d.v_cols // np.uint64(SW)).tolist())) == list(SHARDS)
    assert (d.considered("v", 2) < 0).all() and (d.considered("v", 3) >= 0).all()
    assert len(d.considered("v", 5)) == 1 and len(d.considered("v", 9)) == 0
    cs = cases(d)
    assert len(cs) > 60
    for field, row, nth in cs:
        got = env.q1("i", call_text(field, nth, _filt(row)))
        assert isinstance(got, ValCount)
        assert (got.val, got.count) == oracle(d.considered(field, row), nth), (field, row, nth)


def test_sign_boundary_and_runs_are_hit(env):
    """The generated literals really land where they are meant to."""
    s = np.sort(env.data.considered("v"))
    nneg = int((s < 0).sum())
    lo, hi = nth_for_rank(nneg, len(s)), nth_for_rank(nneg + 1, len(s))
    assert rank(lo, len(s)) == nneg and rank(hi, len(s)) == nneg + 1
    assert env.q1("i", call_text("v", lo)).val < 0 <= env.q1("i", call_text("v", hi)).val
    assert rank("99.9", 2000) == 1998 and rank("0.1", 2000) == 2 and rank("0", 2000) == 1
    # 99.9 as a binary float is a hair above 999/10: exact arithmetic keeps rank 999 of 1000
    assert rank("99.9", 1000) == 999


@pytest.mark.parametrize("field", ["v", "w"])
@pytest.mark.parametrize("filt", ["", "Row(f=1)"])
def test_ends_are_min_and_max(env, field, filt):
    pre = filt + ", " if filt else ""
    assert env.q1("i", call_text(field, "0", filt)).val == env.q1("i", f"Min({pre}field={field})").val
    assert env.q1("i", call_text(field, "100", filt)).val == env.q1("i", f"Max({pre}field={field})").val


@pytest.mark.parametrize("q,msg", [
    ("Percentile(nth=50)", "Percentile(): field required"),
    ("Percentile(field=v)", "Percentile(): nth required"),
    ("Percentile(field=v, nth=true)", "Percentile(): nth must be a number between 0 and 100"),
    ("Percentile(field=v, nth='50')", "Percentile(): nth must be a number between 0 and 100"),
    ("Percentile(field=v, nth=-1)", "Percentile(): nth must be a number between 0 and 100"),
    ("Percentile(field=v, nth=100.5)", "Percentile(): nth must be a number between 0 and 100"),
    ("Percentile(Row(f=1), Row(f=2), field=v, nth=50)", "Percentile() only accepts a single bitmap input"),
])
def test_errors(env, q, msg):
    with pytest.raises(PilosaError) as e:
        env.q("i", q)
    assert str(e.value) == msg


def test_not_an_int_field_and_missing_field(env):
    for q in ("Percentile(field=f, nth=50)", "Percentile(field=nope, nth=50)"):
        got = env.q1("i", q)
        assert (got.val, got.count) == (0, 0)
    assert (lambda r: (r.val, r.count))(env.q1("i", "Sum(field=f)")) == (0, 0)


def test_options_shards(env):
    d = env.data
    for nth in ("0", "50", "99.9"):
        got = env.q1("i", f"Options({call_text('v', nth, 'Row(f=1)')}, shards=[0, 1])")
        assert (got.val, got.count) == oracle(d.considered("v", 1, shards=[0, 1]), nth)
    got = env.q1("i", f"Options({call_text('v', '50')}, shards=[2])")   # only the absent shard
    assert (got.val, got.count) == (0, 0)


def test_parsers_agree():
    """The native parser (pql_parser.cpp, called directly: a missing module
    fails the test) and the Python specification build the same Call."""
    from pilosa_amd import _pql
    from pilosa_amd.pql import Call
    from pilosa_amd.pql import parser as P
    assert P._native is _pql, "parse_string does not use the native parser"
    text = "Percentile(Row(f=1), field=v, nth=99.9)"
    a, b = _pql.parse_calls(text), P.parse_string_py(text).calls
    want = Call("Percentile", {"field": "v", "nth": 99.9}, [Call("Row", {"f": 1})])
    assert list(a) == b == [want] == P.parse_string(text).calls
    assert type(a[0].args["nth"]) is type(b[0].args["nth"]) is float
    text = "Percentile(field=v, nth=50)"
    a, b = _pql.parse_calls(text), P.parse_string_py(text).calls
    assert list(a) == b and type(a[0].args["nth"]) is type(b[0].args["nth"]) is int


def test_protobuf_round_trip():
    from pilosa_amd.server import encoding
    vc = ValCount(-77, 12)
    back = encoding.result_from_pb(encoding.result_to_pb(vc, "Percentile"))
    assert isinstance(back, ValCount) and (back.val, back.count) == (-77, 12)
    assert json.loads(encoding.result_json_bytes(vc)) == {"value": -77, "count": 12}


# ---------------------------------------------------------------- servers
def _req(srv, path, body, headers=None):
    r = urllib.request.Request(f"http://127.0.0.1:{srv.uri.port}{path}", data=body, method="POST",
                               headers=headers or {})
    with urllib.request.urlopen(r, timeout=10) as resp:
        return resp.read()


def _servers(n):
    from pilosa_amd.parallel.cluster import URI
    from pilosa_amd.server.server import Server
    from pilosa_amd.utils.logger import CaptureLogger
    dirs = [tempfile.mkdtemp(prefix="pilosa_amd_test_") for _ in range(n)]
    coord = Server(dirs[0], bind="127.0.0.1:0", node_id="node0", gpu="off", hosts=[], coordinator=True,
                   probe_interval=0.2, logger=CaptureLogger(), hasher="mod")
    if n > 1:
        coord.hosts = [URI.parse("127.0.0.1:1")]  # enable the membership loop
    coord.open()
    servers = [coord]
    for i in range(1, n):
        servers.append(Server(dirs[i], bind="127.0.0.1:0", node_id=f"node{i}", gpu="off",
                              coordinator=False, coordinator_uri=coord.uri.normalize(), probe_interval=0.2,
                              logger=CaptureLogger(), hasher="mod").open())
    deadline = time.time() + 10
    while time.time() < deadline:
        if all(len(s.cluster.nodes) == n and s.cluster.state == "NORMAL" for s in servers):
            break
        time.sleep(0.05)
    for s, d in zip(servers, dirs):
        s.test_dir = d
    states = [(s.node.id, len(s.cluster.nodes), s.cluster.state) for s in servers]
    if not all(k == n and st == "NORMAL" for _, k, st in states):
        _close(servers)
        raise AssertionError(f"the {n}-node cluster did not reach NORMAL: {states}")
    return servers


def _close(servers):
    for s in servers:
        try:
            s.close()
        finally:
            shutil.rmtree(s.test_dir, ignore_errors=True)


def _load_small(servers, seed=5):
    """300 valued columns over shards 0, 1, 3 through Set() calls (routed to
    the owning node); returns {column: value} and the columns of Row(f=1)."""
    from pilosa_amd.server.client import InternalClient
    c = InternalClient()
    s0 = servers[0]
    c.create_index(s0.uri, "i")
    c.create_field(s0.uri, "i", "f", {"type": "set"})
    c.create_field(s0.uri, "i", "v", {"type": "int", "min": -1000, "max": 1000})
    deadline = time.time() + 5
    while time.time() < deadline and not all(s.holder.field("i", "v") is not None for s in servers):
        time.sleep(0.05)
    rng = np.random.default_rng(seed)
    cols = np.concatenate([s * SW + rng.choice(5000, 100, replace=False) for s in SHARDS])
    vals = rng.choice(rng.integers(-1000, 1001, 25), len(cols))
    in_f = cols[rng.random(len(cols)) < 0.5]
    q = " ".join([f"Set({int(col)}, v={int(v)})" for col, v in zip(cols, vals)] +
                 [f"Set({int(col)}, f=1)" for col in in_f])
    assert all(c.query(s0.uri, "i", q)["results"])
    return c, cols, vals.astype(np.int64), in_f


def test_http_json_and_protobuf_results():
    from pilosa_amd.wire import pb
    servers = _servers(1)
    try:
        srv = servers[0]
        c, cols, vals, in_f = _load_small(servers)
        want = oracle(vals[np.isin(cols, in_f)], "99.9")
        body = _req(srv, "/index/i/query", b"Percentile(Row(f=1), field=v, nth=99.9)")
        assert json.loads(body) == {"results": [{"value": want[0], "count": want[1]}]}
        assert b'"value":' in body and b'"count":' in body
        body = _req(srv, "/index/i/query", pb.QueryRequest(Query="Percentile(field=v, nth=50)").SerializeToString(),
                    {"Content-Type": "application/x-protobuf", "Accept": "application/x-protobuf"})
        m = pb.QueryResponse()
        m.ParseFromString(body)
        assert (m.Results[0].ValCount.Val, m.Results[0].ValCount.Count) == oracle(vals, "50")
        got = c.query_node(srv.node, "i", "Percentile(field=v, nth=0)", None)[0]
        assert isinstance(got, ValCount) and (got.val, got.count) == oracle(vals, "0")
    finally:
        _close(servers)


def test_two_node_cluster_matches_single_node():
    servers = _servers(2)
    try:
        single = _servers(1)
    except BaseException:
        _close(servers)
        raise
    try:
        c, cols, vals, in_f = _load_small(servers)
        _load_small(single)
        owners = {s.node.id: sorted(s.holder.field("i", "v").view("bsig_v").fragments) for s in servers}
        assert all(owners.values()) and sorted(sum(owners.values(), [])) == list(SHARDS), owners
        for filt, m in (("", np.ones(len(cols), bool)), ("Row(f=1)", np.isin(cols, in_f))):
            for nth in ["0", "50", "99.9", "100.0"] + boundary_nths(vals[m])[:2]:
                q = call_text("v", nth, filt)
                one = c.query(single[0].uri, "i", q)["results"][0]
                want = oracle(vals[m], nth)
                assert (one["value"], one["count"]) == want, q
                for s in servers:
                    assert c.query(s.uri, "i", q)["results"][0] == one, (q, s.node.id)
    finally:
        _close(servers + single)


# ---------------------------------------------------------------- the chain
def _bit_counts(mags, depth, largest_first, r, tot):
    """cnt1[i] as the device steps produce them: candidates with bit i set
    among those that agree with the decisions on the bits above i."""
    from pilosa_amd.ops.bsi import kth_chain
    cand = np.asarray(mags, dtype=np.int64)
    cnt1 = [0] * depth
    for i in range(depth - 1, -1, -1):
        cnt1[i] = int(((cand >> i) & 1).sum())
        bit, r, tot = kth_chain(largest_first, cnt1[i], r, tot)
        cand = cand[((cand >> i) & 1) == bit]
    return cnt1


def test_chain_replay_against_brute_force():
    rng = np.random.default_rng(7)
    modes = set()
    for trial in range(300):
        depth = int(rng.integers(0, 13))
        n = int(rng.integers(1, 201))
        lim = 1 << depth
        pool = rng.integers(-(lim - 1), lim, size=int(rng.integers(1, 30)))   # duplicates
        if trial % 5 == 0:
            pool = np.abs(pool)
        elif trial % 5 == 1:
            pool = -np.abs(pool) - (pool == 0)
            pool = pool[np.abs(pool) < lim] if (np.abs(pool) < lim).any() else np.array([0])
        vals = rng.choice(pool, n)
        s = np.sort(vals)
        nneg = int((vals < 0).sum())
        for k in sorted({1, n, max(1, nneg), min(n, nneg + 1), int(rng.integers(1, n + 1))}):
            largest, r, tot = kth_plan(k, n, nneg)
            modes.add(largest)
            side = np.abs(vals[vals < 0]) if largest else vals[vals >= 0]
            assert tot == len(side) and 0 <= r < tot
            cnt1 = _bit_counts(side, depth, largest, r, tot)
            mag, count = kth_replay(cnt1, depth, largest, r, tot)
            value = -mag if largest else mag
            assert value == s[k - 1], (trial, k)
            assert count == int((vals == value).sum()), (trial, k)
    assert modes == {True, False}
