"""Distinct(field=): the distinct values of a BSI int field, on the host path.
The reference has no such call, so every answer is pinned to np.unique over
the known values, split by sign; all answers are exact integer sets."""
import json
import os
import tempfile

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import ExecOptions, SignedRow, ValCount
from pilosa_amd.models.row import Row

from tests.distinct_util import call_text, considered, filters, flat, load, oracle, standard_rows
from tests.helpers import SW, Env

SHARDS = (0, 1, 3)   # shard 2 is absent
FIELDS = ("v", "w", "big", "s", "nb")


class Data:
    """1,500 columns over three shards.  v: +-1000 from a pool of 40; w: base
    100, every 5th column without a value; big: depth 40, magnitudes up to
    2^39; s: x and -x both occur, and 0; nb: base -50, so base-relative signs
    and real signs differ (-20 is stored as +30, -50 as 0, -60 as -10)."""
    schema = {"v": dict(min=-1000, max=1000), "w": dict(min=100, max=1100, base=100),
              "big": dict(min=-(1 << 39), max=1 << 39), "s": dict(min=-50, max=50),
              "nb": dict(min=-1000, max=1000, base=-50)}

    def __init__(self, n=1500, seed=31):
        rng = np.random.default_rng(seed)
        per = n // len(SHARDS)
        self.cols = np.concatenate([s * SW + np.sort(rng.choice(SW, per, replace=False))
                                    for s in SHARDS]).astype(np.uint64)
        n = len(self.cols)
        pool_v = np.unique(np.concatenate([[-1000, -1, 0, 1, 1000], rng.integers(-1000, 1001, 35)]))
        big = rng.integers(-(1 << 39) + 1, 1 << 39, n)
        big[:2] = [-(1 << 39), 1 << 39]
        big[2:n // 2] = rng.choice(big[n // 2:n // 2 + 20], n // 2 - 2)   # repeats
        self.vals = {"v": rng.choice(pool_v, n).astype(np.int64),
                     "w": rng.choice(np.unique(rng.integers(100, 1101, 40)), n).astype(np.int64),
                     "big": big.astype(np.int64),
                     "s": rng.choice([-12, -7, -3, 0, 3, 7, 12, 40], n).astype(np.int64),
                     "nb": rng.choice([-1000, -60, -51, -50, -49, -20, -1, 0, 10, 1000], n).astype(np.int64)}
        self.has = {k: np.ones(n, bool) for k in self.vals}
        self.has["w"] = np.arange(n) % 5 != 0
        self.extra = np.array([5, SW + 5, 3 * SW + 5], np.uint64)
        assert not np.isin(self.extra, self.cols).any()
        self.rows = standard_rows(self, rng)


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data()
    load(e, e.data)
    yield e
    e.close()


def test_fixture(env):
    d = env.data
    g = {n: env.holder.field("i", n).bsi_group(n) for n in FIELDS}
    assert g["big"].bit_depth == 40 and int(np.abs(d.vals["big"]).max()) == 1 << 39
    assert g["w"].base == 100 and g["nb"].base == -50 and g["v"].base == 0
    s = set(d.vals["s"].tolist())
    assert 0 in s and all(-x in s for x in s if x not in (0, 40)) and -40 not in s
    # real sign != base-relative sign: -20 is stored as +30
    assert env.holder.fragment("i", "nb", "bsig_nb", 0).distinct(None, g["nb"].bit_depth)[0].tolist().count(30) == 1
    fl = dict(filters(d))
    assert fl["Row(f=5)"].sum() == 1 and not fl["Intersect(Row(f=2), Row(f=3))"].any()
    assert (considered(d, "v", fl["Row(f=2)"]) < 0).all() and (considered(d, "v", fl["Row(f=3)"]) >= 0).all()


@pytest.mark.parametrize("field", FIELDS)
def test_host_path_matches_numpy(env, field):
    d = env.data
    fl = filters(d, other="v" if field == "w" else "w", bound=10 if field == "w" else 500)
    assert len(fl) == 10
    for filt, mask in fl:
        got = env.q1("i", call_text(field, filt))
        assert isinstance(got, SignedRow)
        want = oracle(considered(d, field, mask))
        assert flat(got) == want, (field, filt)
        assert got.values().tolist() == sorted(set(considered(d, field, mask).tolist()))


def test_empty_answers(env):
    for q in ("Distinct(Row(f=9), field=v)", "Distinct(Intersect(Row(f=2), Row(f=3)), field=v)",
              "Options(Distinct(field=v), shards=[2])"):
        got = env.q1("i", q)
        assert isinstance(got, SignedRow) and flat(got) == ([], [])
    env.field("i", "unset", type="int", min=0, max=10)      # no BSI view yet
    assert flat(env.q1("i", "Distinct(field=unset)")) == ([], [])


def test_options_shards_and_remote(env):
    d = env.data
    m = np.isin(d.cols // np.uint64(SW), np.array([1, 3], np.uint64))
    assert flat(env.q1("i", "Options(Distinct(field=v), shards=[1, 3])")) == oracle(considered(d, "v", m))
    got = env.executor.execute("i", "Distinct(field=nb)", opt=ExecOptions(remote=True)).results[0]
    assert flat(got) == oracle(d.vals["nb"])


@pytest.mark.parametrize("q,msg", [
    ("Distinct()", "Distinct(): field required"),
    ("Distinct(Row(f=1))", "Distinct(): field required"),
    ("Distinct(field=nope)", "field not found"),
    ("Distinct(field=f)", 'cannot compute Distinct() on non-integer field: "f"'),
    ("Distinct(field=m)", 'cannot compute Distinct() on non-integer field: "m"'),
    ("Distinct(field=b)", 'cannot compute Distinct() on non-integer field: "b"'),
    ("Distinct(field=t)", 'cannot compute Distinct() on non-integer field: "t"'),
    ("Distinct(Row(f=1), Row(f=2), field=v)", "Distinct() only accepts a single bitmap input"),
    ("Distinct(field=v, k=3)", 'Distinct(): unknown argument "k"'),
    ("Distinct(field=v, nth=50)", 'Distinct(): unknown argument "nth"'),
])
def test_errors(env, q, msg):
    idx = env.holder.index("i")
    for name, opts in (("m", dict(type="mutex")), ("b", dict(type="bool")), ("t", dict(type="time", time_quantum="YMD"))):
        if idx.field(name) is None:
            env.field("i", name, **opts)
    with pytest.raises(PilosaError) as e:
        env.q("i", q)
    assert str(e.value) == msg


def test_field_not_found_is_worded_as_topk_words_it(env):
    errs = []
    for q in ("TopK(field=nope)", "Distinct(field=nope)"):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        errs.append(str(e.value))
    assert errs[0] == errs[1]


def test_nested_use_keeps_the_unknown_call_error(env):
    errs = []
    for q in ("Count(Distinct(field=v))", "Count(NoSuchCall(field=v))"):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        errs.append(str(e.value).replace("NoSuchCall", "Distinct"))
    assert errs[0] == errs[1]


def test_keyed_index_returns_integers_and_no_column_attrs():
    e = Env()
    try:
        e.create_index("k", keys=True)
        e.field("k", "f", keys=True)
        e.field("k", "v", type="int", min=-100, max=100)
        vals = {"a": 7, "b": -7, "c": 0, "d": 7, "e": 1}
        e.q("k", " ".join(f'Set("{c}", v={x})' for c, x in vals.items()) + ' Set("a", f="x") Set("b", f="x")')
        got = e.q1("k", "Distinct(field=v)")
        assert isinstance(got, SignedRow) and flat(got) == ([0, 1, 7], [7])
        assert got.pos.keys is None and got.neg.keys is None
        assert flat(e.q1("k", 'Distinct(Row(f="x"), field=v)')) == ([7], [7])
        assert json.loads(_json(got)) == {"pos": {"attrs": {}, "columns": [0, 1, 7]},
                                          "neg": {"attrs": {}, "columns": [7]}}
        # the column ids 1 .. 5 have attributes; the VALUES 0, 1, 7 must not pick them up
        e.q("k", " ".join(f'SetColumnAttrs("{c}", tag="t{c}")' for c in vals))
        resp = e.executor.execute("k", 'Options(Row(f="x"), columnAttrs=true)')
        assert resp.column_attr_sets, "the fixture's columns carry no attributes"
        resp = e.executor.execute("k", "Options(Distinct(field=v), columnAttrs=true)")
        assert not resp.column_attr_sets and flat(resp.results[0]) == ([0, 1, 7], [7])
    finally:
        e.close()


def _json(r) -> bytes:
    from pilosa_amd.server import encoding
    return encoding.result_json_bytes(r)


def test_json_bytes():
    filled = SignedRow(Row([0, 3, SW + 1]), Row([2]))
    assert _json(filled) == (b'{"pos":{"attrs":{},"columns":[0,3,%d]},"neg":{"attrs":{},"columns":[2]}}' % (SW + 1))
    assert _json(SignedRow()) == b'{"pos":{"attrs":{},"columns":[]},"neg":{"attrs":{},"columns":[]}}'
    # each half is a Row result without attributes, byte for byte
    assert _json(filled) == b'{"pos":' + _json(filled.pos) + b',"neg":' + _json(filled.neg) + b"}"


def test_protobuf_round_trip_and_type_code():
    from pilosa_amd import wire
    from pilosa_amd.server import encoding
    assert wire.QUERY_RESULT_TYPE_SIGNEDROW == 10
    big = SignedRow(Row([0, 5, 1 << 39]), Row([1, 1 << 39]))
    for r in (big, SignedRow(), SignedRow(Row(), Row([9]))):
        m = encoding.result_to_pb(r, "Distinct")
        assert m.Type == 10
        back = encoding.result_from_pb(wire.pb.QueryResult.FromString(m.SerializeToString()))
        assert isinstance(back, SignedRow) and back == r and flat(back) == flat(r)
    m = encoding.result_to_pb(big, "Distinct")
    assert list(m.SignedRow.Pos.Columns) == [0, 5, 1 << 39] and list(m.SignedRow.Neg.Columns) == [1, 1 << 39]
    # Neg = 1, Pos = 2 inside SignedRow = 10; Type = 6
    raw = encoding.result_to_pb(SignedRow(Row([3]), Row([4])), "Distinct").SerializeToString()
    assert raw == bytes.fromhex("300a520a0a030a010412030a0103")
    from pilosa_amd.executor import QueryResponse
    resp = encoding.response_from_pb(encoding.response_to_pb(QueryResponse([big, 3])))
    assert resp.results[0] == big and resp.results[1] == 3


def test_existing_results_keep_their_bytes():
    """Golden bytes written out by hand from the proto: QueryResult{Row = 1,
    ValCount = 5, Type = 6}."""
    from pilosa_amd.server import encoding
    row = encoding.result_to_pb(Row([1, 5, 300]), "Row").SerializeToString()
    assert row == bytes.fromhex("0a06" "0a04" "0105ac02" "3001")
    vc = encoding.result_to_pb(ValCount(-3, 2), "Sum").SerializeToString()
    assert vc == bytes.fromhex("2a0d" "08fdffffffffffffffff01" "1002" "3003")
    assert encoding.result_json_bytes(Row([1, 5, 300])) == b'{"attrs":{},"columns":[1,5,300]}'
    assert encoding.result_json_bytes(ValCount(-3, 2)) == b'{"value":-3,"count":2}'


def test_partial_round_trip():
    from pilosa_amd.parallel.collectives import TAG_ROW, TAG_SIGNED_ROW, decode_partial, encode_partial
    assert TAG_SIGNED_ROW == 12
    for r in (SignedRow(Row([0, 3, SW + 1, 5 * SW + 2, 1 << 39]), Row([2, 3 * SW])), SignedRow(),
              SignedRow(Row(), Row([1]))):
        w = encode_partial(r)
        assert w.dtype == np.int64 and int(w[0]) == TAG_SIGNED_ROW
        back = decode_partial(w)
        assert isinstance(back, SignedRow) and back == r and flat(back) == flat(r)
        # the two rows one after the other in TAG_ROW's segment layout
        assert w[1:].tolist() == encode_partial(r.pos)[1:].tolist() + encode_partial(r.neg)[1:].tolist()
    row = Row([1, SW + 7])
    w = encode_partial(row)
    assert int(w[0]) == TAG_ROW and decode_partial(w) == row


def test_reduce_is_the_union_per_sign():
    a, b = SignedRow(Row([1, 2]), Row([5])), SignedRow(Row([2, SW + 3]), Row([5, 6]))
    assert flat(a.union(b)) == ([1, 2, SW + 3], [5, 6]) == flat(b.union(a))
    assert flat(a.union(SignedRow())) == flat(a)
    assert flat(SignedRow.from_values([3, -4, 3, 0, -4, -(1 << 39), 1 << 39])) == ([0, 3, 1 << 39], [4, 1 << 39])


def test_parsers_agree():
    from pilosa_amd import _pql
    from pilosa_amd.pql import Call
    from pilosa_amd.pql import parser as P
    assert P._native is _pql, "parse_string does not use the native parser"
    text = "Distinct(Intersect(Row(g=1), Not(Row(h=2))), field=v)"
    a, b = _pql.parse_calls(text), P.parse_string_py(text).calls
    want = Call("Distinct", {"field": "v"},
                [Call("Intersect", {}, [Call("Row", {"g": 1}), Call("Not", {}, [Call("Row", {"h": 2})])])])
    assert list(a) == b == [want] == P.parse_string(text).calls
    text = "Distinct(field=v)"
    assert list(_pql.parse_calls(text)) == P.parse_string_py(text).calls == [Call("Distinct", {"field": "v"})]
    for text in ("Distinct(field=v)", "Distinct(Row(f=1), field=v)", "Distinct(Row(v > 10), field=w)"):
        c = P.parse_string(text).calls[0]
        assert P.parse_string(str(c)).calls[0] == c == P.parse_string_py(str(c)).calls[0], str(c)


# ---------------------------------------------------------------- servers
def test_http_json_and_protobuf_results():
    from pilosa_amd.wire import pb
    from tests.test_percentile import _close, _load_small, _req, _servers
    servers = _servers(1)
    try:
        srv = servers[0]
        c, cols, vals, in_f = _load_small(servers)
        pos, neg = oracle(vals[np.isin(cols, in_f)])
        body = _req(srv, "/index/i/query", b"Distinct(Row(f=1), field=v)")
        assert json.loads(body) == {"results": [{"pos": {"attrs": {}, "columns": pos},
                                                 "neg": {"attrs": {}, "columns": neg}}]}
        assert body.index(b'"pos":') < body.index(b'"neg":')
        for q, want in (("Distinct(field=v)", oracle(vals)), ("Distinct(Row(f=7), field=v)", ([], []))):
            body = _req(srv, "/index/i/query", pb.QueryRequest(Query=q).SerializeToString(),
                        {"Content-Type": "application/x-protobuf", "Accept": "application/x-protobuf"})
            m = pb.QueryResponse()
            m.ParseFromString(body)
            assert m.Results[0].Type == 10, q
            assert (list(m.Results[0].SignedRow.Pos.Columns), list(m.Results[0].SignedRow.Neg.Columns)) == want
        got = c.query_node(srv.node, "i", "Distinct(field=v)", None)[0]
        assert isinstance(got, SignedRow) and flat(got) == oracle(vals)
    finally:
        _close(servers)


def test_two_node_cluster_matches_single_node():
    from tests.test_percentile import _close, _load_small, _servers
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
        for filt, m in (("", np.ones(len(cols), bool)), ("Row(f=1)", np.isin(cols, in_f)),
                        ("Row(f=7)", np.zeros(len(cols), bool))):
            q = call_text("v", filt)
            one = c.query(single[0].uri, "i", q)["results"][0]
            pos, neg = oracle(vals[m])
            assert one == {"pos": {"attrs": {}, "columns": pos}, "neg": {"attrs": {}, "columns": neg}}, q
            for s in servers:
                assert c.query(s.uri, "i", q)["results"][0] == one, (q, s.node.id)
    finally:
        _close(servers + single)


# ---------------------------------------------------------------- mesh
MESH_QUERIES = ["Distinct(field=v)", "Distinct(Row(f=1), field=v)", "Distinct(Not(Row(g=3)), field=v)",
                "Distinct(Row(g=9), field=v)"]


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
    last = {}
    for col, v in vals:
        last[col] = v
    pos, neg = oracle(list(last.values()))
    first = json.loads(want[0])[0]
    assert first["pos"]["columns"] == pos and first["neg"]["columns"] == neg and pos and neg
    assert json.loads(want[3])[0] == {"pos": {"attrs": {}, "columns": []}, "neg": {"attrs": {}, "columns": []}}
