"""TopK(field=, k=): the exact top rows of a field, on the host path.  The
reference has no such call, so every answer is pinned to counts computed with
numpy from the generated columns; all answers are exact integers."""
import json
import os
import tempfile

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.models.cache import Pair

from tests.helpers import SW, Env
from tests.test_percentile import _close, _req, _servers
from tests.topk_util import A_IDS, BIG_ROW, FILTERS, KS, N_IDS, SHARDS, Data, call_text, flat


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data()
    e.data.load(e)
    yield e
    e.close()


def test_fixture(env):
    d = env.data
    assert len(A_IDS) == 70 and len(set(A_IDS)) == 70 and max(A_IDS) >= 1 << 40
    assert sorted(set((d.cols // np.uint64(SW)).tolist())) == list(SHARDS)
    allr = d.expected("a")
    assert len(allr) == 70
    counts = [n for _, n in allr]
    assert len(counts) - len(set(counts)) >= 2, "the fixture holds no ties"
    assert not ((d.cols[d.rows["a"][A_IDS[3]]] // np.uint64(SW)) == 1).any()     # absent from shard 1
    for filt in FILTERS[1:]:
        assert A_IDS[4] not in dict(d.expected("a", filt))                        # meets no filter
    assert d.expected("a", "Row(f=9)") == []


@pytest.mark.parametrize("filt", FILTERS)
def test_host_path_matches_numpy(env, filt):
    d = env.data
    for field in ("a", "n"):
        for k in KS:
            got = env.q1("i", call_text(field, filt, k))
            assert isinstance(got, list) and all(isinstance(p, Pair) for p in got)
            assert flat(got) == d.expected(field, filt, k), (field, filt, k)
    if filt != "Row(f=9)":
        assert len(d.expected("a", filt)) >= 60 and len(d.expected("a", filt, 5)) == 5


def test_tie_order_is_by_row_id(env):
    got = flat(env.q1("i", call_text("a", "Row(f=1)")))
    pos = {r: i for i, (r, _) in enumerate(got)}
    cnt = dict(got)
    for lo, hi in ((A_IDS[5], A_IDS[6]), (A_IDS[7], A_IDS[8])):
        assert cnt[lo] == cnt[hi] and pos[hi] == pos[lo] + 1
    assert got == sorted(got, key=lambda p: (-p[1], p[0]))
    assert cnt[BIG_ROW] > 0


@pytest.mark.parametrize("q,msg", [
    ("TopK(k=3)", "TopK(): field required"),
    ("TopK(field=7)", "TopK(): field required"),
    ("TopK(field=w)", 'cannot compute TopK() on integer field: "w"'),
    ("TopK(field=nope)", "field not found"),
    ("TopK(field=a, k=-1)", "TopK(): k must be a non-negative integer"),
    ("TopK(field=a, k=true)", "TopK(): k must be a non-negative integer"),
    ("TopK(field=a, k='3')", "TopK(): k must be a non-negative integer"),
    ("TopK(field=a, k=1.5)", "TopK(): k must be a non-negative integer"),
    ("TopK(Row(f=1), Row(g=1), field=a)", "TopK() only accepts a single bitmap input"),
    ("TopK(field=a, from='2010-01-01T00:00')", 'TopK(): unknown argument "from"'),
    ("TopK(field=a, to='2010-01-01T00:00')", 'TopK(): unknown argument "to"'),
    ("TopK(field=a, threshold=2)", 'TopK(): unknown argument "threshold"'),
    ("TopK(field=a, n=2)", 'TopK(): unknown argument "n"'),
])
def test_errors(env, q, msg):
    with pytest.raises(PilosaError) as e:
        env.q("i", q)
    assert str(e.value) == msg


def test_field_not_found_is_the_usual_error(env):
    from pilosa_amd.errors import ErrFieldNotFound
    with pytest.raises(PilosaError) as e:
        env.q("i", "TopK(field=nope)")
    with pytest.raises(PilosaError) as rows:
        env.q("i", "Rows(nope)")
    assert str(e.value) == str(rows.value) == str(ErrFieldNotFound)


def test_cache_type_none_field(env):
    d = env.data
    assert env.holder.field("i", "n").options.cache_type == "none"
    assert flat(env.q1("i", "TopK(field=n)")) == d.expected("n") and len(d.expected("n")) == len(N_IDS)
    assert flat(env.q1("i", "TopK(Row(g=1), field=n, k=2)")) == [
        p for p in sorted(((r, int((m & d.rows["g"][1]).sum())) for r, m in d.rows["n"].items()),
                          key=lambda p: (-p[1], p[0])) if p[1]][:2]
    with pytest.raises(PilosaError) as e:      # TopN on it raises as before
        env.q("i", "TopN(n, Row(g=1), n=2)")
    assert str(e.value) == 'cannot compute TopN(), field has no cache: "n"'


def test_never_touches_a_rank_cache(env):
    frags = env.holder.view("i", "a", "standard").all_fragments()

    from pilosa_amd.models.cache import RankCache
    assert frags and all(isinstance(f.cache, RankCache) for f in frags)

    def state():
        return [(len(f.cache), f.cache.version, f.cache.update_time) for f in frags]
    before = state()
    for f in frags:
        f.cache.update_time = before[0][2] - 3600      # a read of the cache would re-rank it now
    before = state()
    env.q("i", "TopK(Row(f=1), field=a, k=3)")
    assert state() == before


def test_options_shards(env):
    d = env.data
    for filt in ("", "Row(f=1)"):
        got = env.q1("i", f"Options({call_text('a', filt, 7)}, shards=[1, 3])")
        assert flat(got) == d.expected("a", filt, 7, shards=[1, 3])
    assert A_IDS[3] not in dict(flat(env.q1("i", f"Options({call_text('a')}, shards=[1])")))
    assert env.q1("i", f"Options({call_text('a')}, shards=[2])") == []      # only the absent shard


def test_remote_returns_every_pair(env):
    """A node answering for a coordinator must not cut: exactness needs all
    its partials."""
    from pilosa_amd.executor import ExecOptions
    got = env.executor.execute("i", call_text("a", "Row(f=1)", 1), opt=ExecOptions(remote=True)).results[0]
    assert flat(got) == env.data.expected("a", "Row(f=1)")


def test_parsers_agree():
    from pilosa_amd import _pql
    from pilosa_amd.pql import Call
    from pilosa_amd.pql import parser as P
    assert P._native is _pql, "parse_string does not use the native parser"
    text = "TopK(Intersect(Row(g=1), Not(Row(h=2))), field=f, k=10)"
    a, b = _pql.parse_calls(text), P.parse_string_py(text).calls
    want = Call("TopK", {"field": "f", "k": 10},
                [Call("Intersect", {}, [Call("Row", {"g": 1}), Call("Not", {}, [Call("Row", {"h": 2})])])])
    assert list(a) == b == [want] == P.parse_string(text).calls
    text = "TopK(field=f)"
    assert list(_pql.parse_calls(text)) == P.parse_string_py(text).calls == [Call("TopK", {"field": "f"})]


def test_encodings():
    from pilosa_amd.server import encoding
    pairs = [Pair(BIG_ROW, 9), Pair(3, 9), Pair(1, 2)]
    m = encoding.result_to_pb(pairs, "TopK")
    assert m.Type == encoding.QUERY_RESULT_TYPE_PAIRS
    assert flat(encoding.result_from_pb(m)) == flat(pairs)
    assert json.loads(encoding.result_json_bytes(pairs)) == [{"id": BIG_ROW, "count": 9}, {"id": 3, "count": 9},
                                                             {"id": 1, "count": 2}]
    empty = encoding.result_to_pb([], "TopK")
    assert empty.Type == encoding.QUERY_RESULT_TYPE_PAIRS != encoding.QUERY_RESULT_TYPE_ROWIDS
    assert encoding.result_from_pb(empty) == []
    assert json.loads(encoding.result_json_bytes([])) == []


def test_partial_round_trip():
    from pilosa_amd.parallel.collectives import TAG_PAIRS, decode_partial, encode_partial
    pairs = [Pair(BIG_ROW, 1 << 33), Pair(0, 1), Pair(17, 5)]
    w = encode_partial(pairs)
    assert int(w[0]) == TAG_PAIRS and flat(decode_partial(w)) == flat(pairs)
    w = encode_partial([])
    assert decode_partial(w) == []


def test_keyed_field_returns_keys():
    e = Env()
    try:
        e.create_index("k", keys=True)
        e.field("k", "tag", keys=True)
        e.field("k", "f", keys=True)
        q = " ".join(f'Set("c{c}", tag="{t}")' for t, n in (("red", 5), ("blue", 9), ("green", 5), ("grey", 1))
                     for c in range(n))
        e.q("k", q + ' Set("c0", f="x") Set("c1", f="x") Set("c7", f="x")')
        got = e.q1("k", "TopK(field=tag)")
        assert [(p.key, p.count, p.id) for p in got] == [("blue", 9, 0), ("red", 5, 0), ("green", 5, 0),
                                                         ("grey", 1, 0)]
        got = e.q1("k", 'TopK(Row(f="x"), field=tag, k=2)')
        assert [(p.key, p.count) for p in got] == [("blue", 3), ("red", 2)]
        assert e.q1("k", 'TopK(Row(f="nobody"), field=tag)') == []
    finally:
        e.close()


# ---------------------------------------------------------------- servers
def _load_small(servers, seed=9):
    """Rows 1 .. 12 of a (row r on about r/14 of 300 columns over shards 0, 1,
    3) and f=1 on a random half, through Set() calls routed to the owners."""
    from pilosa_amd.server.client import InternalClient
    import time
    c = InternalClient()
    s0 = servers[0]
    c.create_index(s0.uri, "i")
    c.create_field(s0.uri, "i", "a", {"type": "set", "cacheType": "none"})
    c.create_field(s0.uri, "i", "f", {"type": "set"})
    deadline = time.time() + 5
    while time.time() < deadline and not all(s.holder.field("i", "f") is not None for s in servers):
        time.sleep(0.05)
    rng = np.random.default_rng(seed)
    cols = np.concatenate([s * SW + rng.choice(5000, 100, replace=False) for s in SHARDS])
    member = {r: cols[rng.random(len(cols)) < r / 14] for r in range(1, 13)}
    member[12] = member[11]                                    # a tie
    in_f = cols[rng.random(len(cols)) < 0.5]
    q = " ".join([f"Set({int(col)}, a={r})" for r, cc in member.items() for col in cc] +
                 [f"Set({int(col)}, f=1)" for col in in_f])
    assert c.query(s0.uri, "i", q)["results"]
    return c, member, in_f


def _want(member, keep=None, k=None):
    out = [(r, int(len(cc) if keep is None else np.isin(cc, keep).sum())) for r, cc in member.items()]
    out = sorted((p for p in out if p[1]), key=lambda p: (-p[1], p[0]))
    return [{"id": r, "count": n} for r, n in (out[:k] if k else out)]


def test_http_json_and_protobuf_results():
    from pilosa_amd.wire import pb
    servers = _servers(1)
    try:
        srv = servers[0]
        c, member, in_f = _load_small(servers)
        body = _req(srv, "/index/i/query", b"TopK(Row(f=1), field=a, k=4)")
        assert json.loads(body) == {"results": [_want(member, in_f, 4)]}
        for q, want in (("TopK(field=a, k=3)", _want(member, None, 3)), ("TopK(Row(f=7), field=a)", [])):
            body = _req(srv, "/index/i/query", pb.QueryRequest(Query=q).SerializeToString(),
                        {"Content-Type": "application/x-protobuf", "Accept": "application/x-protobuf"})
            m = pb.QueryResponse()
            m.ParseFromString(body)
            from pilosa_amd.server import encoding
            assert m.Results[0].Type == encoding.QUERY_RESULT_TYPE_PAIRS, q
            assert [{"id": p.ID, "count": p.Count} for p in m.Results[0].Pairs] == want
        got = c.query_node(srv.node, "i", "TopK(Row(f=7), field=a)", None)[0]
        assert got == []
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
        c, member, in_f = _load_small(servers)
        _load_small(single)
        owners = {s.node.id: sorted(s.holder.field("i", "a").view("standard").fragments) for s in servers}
        assert all(owners.values()) and sorted(sum(owners.values(), [])) == list(SHARDS), owners
        for filt, keep in (("", None), ("Row(f=1), ", in_f)):
            for k in (None, 1, 5, 100):
                q = f"TopK({filt}field=a" + (f", k={k})" if k is not None else ")")
                one = c.query(single[0].uri, "i", q)["results"][0]
                assert one == _want(member, keep, k), q
                for s in servers:
                    assert c.query(s.uri, "i", q)["results"][0] == one, (q, s.node.id)
    finally:
        _close(servers + single)


# ---------------------------------------------------------------- mesh
MESH_QUERIES = ["TopK(field=f)", "TopK(field=f, k=2)", "TopK(Row(g=3), field=f)", "TopK(Row(g=3), field=g, k=1)",
                "TopK(Not(Row(f=1)), field=g)", "TopK(Row(g=9), field=f)"]


def _mesh_worker(rank, world, port, outdir):
    import torch.distributed as dist

    from pilosa_amd.executor import Executor
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.parallel.mesh import ShardMesh
    from tests.test_mesh import _canon, _data, _load, _setup_schema

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    holder = Holder(tempfile.mkdtemp(prefix=f"mesh{rank}_")).open()
    ex = Executor(holder)
    mesh = ShardMesh(ex, block=1)
    ex.mesh = mesh
    try:
        if rank != 0:
            mesh.serve()
            return
        _setup_schema(holder)
        mesh.apply_schema()
        bits, vals = _data()
        _load(ex, bits, vals, mesh)
        got = [_canon(ex.execute("i", q).results) for q in MESH_QUERIES]
        with open(os.path.join(outdir, "mesh.json"), "w") as fh:
            json.dump({"got": got}, fh)
        mesh.stop()
    finally:
        ex.close()
        holder.close()
        dist.destroy_process_group()


def test_two_rank_mesh_equals_host(tmp_path):
    import torch.multiprocessing as mp

    from pilosa_amd.executor import Executor
    from pilosa_amd.models.holder import Holder
    from tests.helpers import free_port
    from tests.test_mesh import _canon, _data, _load, _setup_schema

    mp.start_processes(_mesh_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    res = json.load(open(tmp_path / "mesh.json"))
    holder = Holder(tempfile.mkdtemp(prefix="mesh_ref_")).open()
    ex = Executor(holder)
    try:
        _setup_schema(holder)
        bits, vals = _data()
        _load(ex, bits, vals)
        want = [_canon(ex.execute("i", q).results) for q in MESH_QUERIES]
    finally:
        ex.close()
        holder.close()
    for q, g, w in zip(MESH_QUERIES, res["got"], want):
        assert g == w, q
    assert json.loads(want[1])[0] and len(json.loads(want[1])[0]) == 2 and json.loads(want[5]) == [[]]
