"""Sort(field=, limit=, offset=, sort-desc=): columns ordered by an int field,
on the host path.  Pilosa v1.3 has no such call, so every answer is pinned to
np.lexsort over the known values (value, then column); all answers are exact."""
import json
import os
import tempfile

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import ExecOptions, ExtractedTable, SignedRow, SortedColumns, ValCount
from pilosa_amd.models.row import Row

from tests.distinct_util import filters, load
from tests.helpers import SW, Env
from tests.sort_util import call_text, check, cut_limits, oracle, tie_group, window
from tests.test_distinct import SHARDS, Data

INT_FIELDS = ("v", "w", "big", "nb", "s")   # +-, a base, depth 40, a negative base, few distinct values


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data()
    load(e, e.data)
    yield e
    e.close()


def test_fixture(env):
    d = env.data
    g = {n: env.holder.field("i", n).bsi_group(n) for n in INT_FIELDS}
    assert g["big"].bit_depth == 40 and g["w"].base == 100 and g["nb"].base == -50
    assert (d.vals["v"] < 0).any() and (d.vals["v"] > 0).any() and not d.has["w"].all()
    lo, hi = tie_group(oracle(d, "s", np.ones(len(d.cols), bool))[1])
    assert hi - lo > 100, "s has no large tie group"
    assert sorted(set((d.cols // np.uint64(SW)).tolist())) == list(SHARDS)


@pytest.mark.parametrize("field", INT_FIELDS)
def test_fields_and_filters_match_numpy(env, field):
    d = env.data
    fl = filters(d, other="v" if field == "w" else "w", bound=10 if field == "w" else 500)
    assert len(fl) == 10
    for filt, mask in fl:
        for desc in (False, True):
            want = oracle(d, field, mask, desc)
            for lim in (None, 7):
                got = env.q1("i", call_text(field, filt, limit=lim, desc=desc if desc else None))
                assert isinstance(got, SortedColumns) and got.keys is None
                check(got, window(want, 0, lim), (filt, desc, lim))
    assert len(env.q1("i", call_text(field, "Row(f=9)"))) == 0            # a row that does not exist
    assert len(env.q1("i", call_text(field, "Intersect(Row(f=2), Row(f=3))"))) == 0


def test_explicit_ascending_is_the_default(env):
    assert env.q1("i", call_text("v", "Row(f=1)", limit=20, desc=False)) == \
        env.q1("i", call_text("v", "Row(f=1)", limit=20))


@pytest.mark.parametrize("desc", [False, True])
def test_limit_cuts_a_tie_group_at_its_first_middle_and_last_member(env, desc):
    d = env.data
    for field, filt, mask in (("s", "", np.ones(len(d.cols), bool)), ("s", "Row(f=1)", d.rows[1]),
                              ("nb", "Not(Row(f=1))", ~d.rows[1])):
        want = oracle(d, field, mask, desc)
        n = len(want[0])
        lo, hi = tie_group(want[1])
        assert hi - lo >= 3 and len({int(c) // SW for c in want[0][lo:hi]}) > 1, "the tie group lies in one shard"
        limits = cut_limits(want[1])
        assert {0, 1, n - 1, n, n + 1, lo + 1, (lo + hi) // 2, hi} <= set(limits)
        for lim in limits:
            check(env.q1("i", call_text(field, filt, limit=lim, desc=desc)), window(want, 0, lim), (field, lim))
        # ties go by column id ascending in both directions
        got = env.q1("i", call_text(field, filt, limit=hi, desc=desc))
        assert (np.diff(got.columns[lo:hi].astype(np.int64)) > 0).all()


def test_offsets_inside_and_past_the_answer(env):
    d = env.data
    for desc in (False, True):
        want = oracle(d, "v", d.rows[1], desc)
        n = len(want[0])
        for off, lim in ((0, 5), (3, 5), (n - 2, 5), (n, 5), (n + 4, None), (10, None), (7, 0), (0, None)):
            q = call_text("v", "Row(f=1)", limit=lim, offset=off, desc=desc)
            check(env.q1("i", q), window(want, off, lim), q)
        # no filter
        check(env.q1("i", call_text("v", limit=9, offset=4, desc=desc)),
              window(oracle(d, "v", np.ones(len(d.cols), bool), desc), 4, 9))


def test_options_shards_and_remote_keeps_the_offset(env):
    d = env.data
    want = oracle(d, "v", d.rows[1] & (d.cols // np.uint64(SW) == np.uint64(1)))
    got = env.q1("i", f"Options({call_text('v', 'Row(f=1)', limit=4, offset=2)}, shards=[1])")
    check(got, window(want, 2, 4))
    # a node answering for a coordinator returns its first offset + limit entries
    r = env.executor.execute("i", call_text("v", "Row(f=1)", limit=4, offset=2), shards=[1],
                             opt=ExecOptions(remote=True)).results[0]
    check(r, window(want, 0, 6))


def test_missing_view_and_fragment(env):
    env.field("i", "fresh", type="int", min=-5, max=5)
    assert env.q1("i", "Sort(field=fresh)") == SortedColumns()
    assert env.q1("i", "Sort(Row(f=1), field=fresh, limit=3)") == SortedColumns()
    # a value in one shard only: the other shards have no fragment
    env.q("i", f"Set({SW + 5}, fresh=-2)")
    got = env.q1("i", "Sort(field=fresh, sort-desc=true)")
    assert got.columns.tolist() == [SW + 5] and got.values.tolist() == [-2]


@pytest.mark.parametrize("q,msg", [
    ("Sort()", "Sort(): field required"),
    ("Sort(Row(f=1))", "Sort(): field required"),
    ("Sort(field=1)", "Sort(): field required"),
    ("Sort(field=f)", 'cannot compute Sort() on non-integer field: "f"'),
    ("Sort(Row(f=1), Row(f=2), field=v)", "Sort() only accepts a single bitmap input"),
    ("Sort(field=v, limit=-1)", "Sort(): limit must be a non-negative integer"),
    ("Sort(field=v, limit=1.5)", "Sort(): limit must be a non-negative integer"),
    ("Sort(field=v, limit=true)", "Sort(): limit must be a non-negative integer"),
    ("Sort(field=v, offset=-2)", "Sort(): offset must be a non-negative integer"),
    ('Sort(field=v, offset="3")', "Sort(): offset must be a non-negative integer"),
    ("Sort(field=v, sort-desc=1)", "Sort(): sort-desc must be a boolean"),
    ('Sort(field=v, sort-desc="true")', "Sort(): sort-desc must be a boolean"),
    ("Sort(field=v, nth=5)", 'Sort(): unknown argument "nth"'),
    ("Sort(field=v, sortdesc=true)", 'Sort(): unknown argument "sortdesc"'),
])
def test_errors(env, q, msg):
    with pytest.raises(PilosaError) as e:
        env.q("i", q)
    assert str(e.value) == msg


def test_field_not_found_is_worded_as_distinct_words_it(env):
    errs = []
    for q in ("Distinct(field=nope)", "Sort(field=nope)"):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        errs.append(str(e.value))
    assert errs[0] == errs[1]


def test_nested_use_keeps_the_unknown_call_error(env):
    errs = []
    for q in ("Count(Sort(field=v))", "Count(NoSuchCall(field=v))"):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        errs.append(str(e.value).replace("NoSuchCall", "Sort"))
    assert errs[0] == errs[1]


def test_size_guard(env, monkeypatch):
    d = env.data
    want = oracle(d, "v", d.rows[1])
    monkeypatch.setenv("PILOSA_SORT_MAX_COLUMNS", "10")
    gathered = []
    from pilosa_amd.models.fragment import Fragment
    real = Fragment.sort_values
    monkeypatch.setattr(Fragment, "sort_values", lambda self, *a: gathered.append(1) or real(self, *a))
    for q, n in ((call_text("v", "Row(f=1)"), len(want[0])),
                 (call_text("v"), int(d.has["v"].sum())),
                 (call_text("v", "Row(f=1)", offset=8, limit=3), 11),
                 (call_text("v", "Row(f=5)", offset=11, limit=0), 11)):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        assert str(e.value) == f"Sort(): {n} columns exceed the limit of 10; page with limit= and offset="
    assert not gathered, "the guard ran after values were gathered"
    check(env.q1("i", call_text("v", "Row(f=1)", offset=7, limit=3)), window(want, 7, 3))
    check(env.q1("i", call_text("v", "Row(f=5)")), oracle(d, "v", d.rows[5]))     # one considered column
    assert gathered
    # w lacks a value in every 5th column: the guard counts the considered columns, not the filter's
    monkeypatch.setenv("PILOSA_SORT_MAX_COLUMNS", str(int((d.has["w"] & d.rows[1]).sum())))
    check(env.q1("i", call_text("w", "Row(f=1)")), oracle(d, "w", d.rows[1]))
    assert int(d.rows[1].sum()) > int((d.has["w"] & d.rows[1]).sum())


# ---------------------------------------------------------------- the result type
def _json(r) -> bytes:
    from pilosa_amd.server import encoding
    return encoding.result_json_bytes(r)


def _sample():
    return SortedColumns(np.array([SW + 2, 1, 5], np.uint64), np.array([-7, 0, 9], np.int64))


def test_json_bytes():
    assert _json(_sample()) == b'{"columns":[%d,1,5],"values":[-7,0,9]}' % (SW + 2)
    assert _json(SortedColumns()) == b'{"columns":[],"values":[]}'
    keyed = SortedColumns(np.array([3, 4], np.uint64), np.array([2, 2], np.int64), ["c3", "c4"])
    assert _json(keyed) == b'{"keys":["c3","c4"],"values":[2,2]}'


def test_equality_slice_merge_and_repr():
    a, b = _sample(), _sample()
    assert a == b and not (a != b) and a != SignedRow() and a != a.slice(0, 2) and len(a) == 3
    b.values[0] = 8
    assert a != b
    assert repr(a) == "SortedColumns(columns=3)"
    assert a.slice(1).columns.tolist() == [1, 5] and a.slice(1, 2).values.tolist() == [0]
    x = SortedColumns(np.array([4, 9], np.uint64), np.array([1, 5], np.int64))
    y = SortedColumns(np.array([2, 3, 7], np.uint64), np.array([1, 5, 5], np.int64))
    m = x.merge(y, None, False)
    assert m.columns.tolist() == [2, 4, 3, 7, 9] and m.values.tolist() == [1, 1, 5, 5, 5]
    xd = SortedColumns(x.columns[::-1], x.values[::-1])
    yd = SortedColumns(np.array([3, 7, 2], np.uint64), np.array([5, 5, 1], np.int64))
    m = xd.merge(yd, 4, True)
    assert m.columns.tolist() == [3, 7, 9, 2] and m.values.tolist() == [5, 5, 5, 1]
    lo, hi = -(1 << 63), (1 << 63) - 1
    ext = SortedColumns(np.array([1, 2], np.uint64), np.array([lo, hi], np.int64))
    assert ext.merge(SortedColumns(), None, True).values.tolist() == [hi, lo]


def test_protobuf_round_trip_and_type_code():
    from pilosa_amd import wire
    from pilosa_amd.executor import QueryResponse
    from pilosa_amd.server import encoding
    assert wire.QUERY_RESULT_TYPE_SORTEDCOLUMNS == 12
    keyed = SortedColumns(np.array([3, 4], np.uint64), np.array([2, -2], np.int64), ["c3", "c4"])
    for r in (_sample(), SortedColumns(), keyed):
        m = encoding.result_to_pb(r, "Sort")
        assert m.Type == 12
        back = encoding.result_from_pb(wire.pb.QueryResult.FromString(m.SerializeToString()))
        assert isinstance(back, SortedColumns) and back == r
        assert back.columns.dtype == np.uint64 and back.values.dtype == np.int64
    # SortedColumns = 12 (0x62), Columns = 1 and Values = 3 packed, Type = 6 (0x30)
    raw = encoding.result_to_pb(SortedColumns(np.array([3, 300], np.uint64), np.array([4, -1], np.int64)),
                                "Sort").SerializeToString()
    assert raw == bytes.fromhex("300c" "6212" "0a03" "03ac02" "1a0b" "04" "ffffffffffffffffff01")
    raw = encoding.result_to_pb(keyed, "Sort").SerializeToString()
    assert bytes.fromhex("12026333" "12026334") in raw                      # Keys = 2
    resp = encoding.response_from_pb(encoding.response_to_pb(QueryResponse([_sample(), 3])))
    assert resp.results[0] == _sample() and resp.results[1] == 3


def test_existing_results_keep_their_bytes():
    """Golden bytes written out by hand from the proto: QueryResult{Row = 1,
    ValCount = 5, SignedRow = 10, ExtractedTable = 11, Type = 6}."""
    from pilosa_amd.server import encoding
    row = encoding.result_to_pb(Row([1, 5, 300]), "Row").SerializeToString()
    assert row == bytes.fromhex("0a06" "0a04" "0105ac02" "3001")
    vc = encoding.result_to_pb(ValCount(-3, 2), "Sum").SerializeToString()
    assert vc == bytes.fromhex("2a0d" "08fdffffffffffffffff01" "1002" "3003")
    sr = encoding.result_to_pb(SignedRow(Row([3]), Row([4])), "Distinct").SerializeToString()
    assert sr == bytes.fromhex("300a520a0a030a010412030a0103")
    et = encoding.result_to_pb(ExtractedTable([("v", "int64")], np.array([3], np.uint64),
                                              [(np.array([4], np.int64), np.array([True]))]),
                               "Extract").SerializeToString()
    assert et == bytes.fromhex("300b" "5a15" "0a10""0a0176" "1205696e743634" "1a0104" "320101" "120103")
    assert encoding.result_json_bytes(Row([1, 5, 300])) == b'{"attrs":{},"columns":[1,5,300]}'
    assert encoding.result_json_bytes(ValCount(-3, 2)) == b'{"value":-3,"count":2}'
    assert encoding.result_json_bytes(SignedRow(Row([3]), Row([4]))) == \
        b'{"pos":{"attrs":{},"columns":[3]},"neg":{"attrs":{},"columns":[4]}}'
    assert encoding.result_json_bytes(ExtractedTable([("v", "int64")])) == \
        b'{"fields":[{"name":"v","type":"int64"}],"columns":[]}'


def test_partial_round_trip():
    from pilosa_amd.parallel.collectives import TAG_EXTRACT, TAG_ROW, TAG_SORTED, decode_partial, encode_partial
    assert TAG_SORTED == 14 and TAG_EXTRACT == 13
    big = SortedColumns(np.array([(1 << 64) - 1, 1 << 40], np.uint64), np.array([-(1 << 63), (1 << 63) - 1], np.int64))
    for r in (_sample(), SortedColumns(), big):
        w = encode_partial(r)
        assert w.dtype == np.int64 and int(w[0]) == TAG_SORTED and len(w) == 2 + 2 * len(r)
        back = decode_partial(w)
        assert isinstance(back, SortedColumns) and back == r
        assert back.columns.dtype == np.uint64 and back.values.dtype == np.int64
    row = Row([1, SW + 7])
    w = encode_partial(row)
    assert int(w[0]) == TAG_ROW and decode_partial(w) == row


def test_parsers_agree():
    from pilosa_amd import _pql
    from pilosa_amd.pql import Call
    from pilosa_amd.pql import parser as P
    assert P._native is _pql, "parse_string does not use the native parser"
    text = "Sort(Intersect(Row(g=1), Not(Row(h=2))), field=v, limit=10, offset=3, sort-desc=true)"
    a, b = _pql.parse_calls(text), P.parse_string_py(text).calls
    want = Call("Sort", {"field": "v", "limit": 10, "offset": 3, "sort-desc": True},
                [Call("Intersect", {}, [Call("Row", {"g": 1}), Call("Not", {}, [Call("Row", {"h": 2})])])])
    assert list(a) == b == [want] == P.parse_string(text).calls
    for text in ("Sort(field=v)", "Sort(Row(v > 10), field=w, sort-desc=false, limit=2)",
                 "Sort(field=v, sort-desc=true)"):
        c = P.parse_string(text).calls[0]
        assert P.parse_string(str(c)).calls[0] == c == P.parse_string_py(str(c)).calls[0], str(c)


def test_keyed_index_and_column_attrs():
    e = Env()
    try:
        e.create_index("k", keys=True)
        e.field("k", "f", keys=True)
        e.field("k", "v", type="int", min=-100, max=100)
        vals = {"a": 7, "b": -7, "c": 0, "d": 7}
        e.q("k", " ".join(f'Set("{c}", v={x})' for c, x in vals.items()) +
            ' Set("a", f="x") Set("b", f="x") Set("e", f="x") Set("d", f="x")')
        got = e.q1("k", "Sort(field=v)")
        assert got.keys == ["b", "c", "a", "d"] and got.values.tolist() == [-7, 0, 7, 7]
        got = e.q1("k", 'Sort(Row(f="x"), field=v, sort-desc=true)')
        assert got.keys == ["a", "d", "b"] and got.values.tolist() == [7, 7, -7]           # values are never translated
        assert json.loads(_json(got)) == {"keys": ["a", "d", "b"], "values": [7, 7, -7]}
        assert e.q1("k", 'Sort(Row(f="x"), field=v, limit=1, offset=1)').keys == ["a"]
        e.q("k", " ".join(f'SetColumnAttrs("{c}", tag="t{c}")' for c in vals))
        resp = e.executor.execute("k", 'Options(Row(f="x"), columnAttrs=true)')
        assert resp.column_attr_sets, "the fixture's columns carry no attributes"
        resp = e.executor.execute("k", 'Options(Sort(Row(f="x"), field=v), columnAttrs=true)')
        assert not resp.column_attr_sets and resp.results[0].keys == ["b", "a", "d"]
    finally:
        e.close()


# ---------------------------------------------------------------- servers
WINDOWS = [(None, None), (0, 7), (5, 40), (120, 50), (140, None), (0, 0)]


def _small_oracle(cols, vals, mask, desc):
    c, v = cols[mask].astype(np.uint64), vals[mask]
    order = np.lexsort((c, ~v if desc else v))
    return c[order], v[order]


def test_http_json_and_protobuf_results():
    from pilosa_amd.wire import pb
    from tests.test_percentile import _close, _load_small, _req, _servers
    servers = _servers(1)
    try:
        srv = servers[0]
        c, cols, vals, in_f = _load_small(servers)
        wc, wv = _small_oracle(cols, vals, np.isin(cols, in_f), True)
        body = _req(srv, "/index/i/query", b"Sort(Row(f=1), field=v, sort-desc=true)")
        assert json.loads(body) == {"results": [{"columns": wc.tolist(), "values": wv.tolist()}]}
        body = _req(srv, "/index/i/query",
                    pb.QueryRequest(Query="Sort(Row(f=1), field=v, sort-desc=true, limit=3)").SerializeToString(),
                    {"Content-Type": "application/x-protobuf", "Accept": "application/x-protobuf"})
        m = pb.QueryResponse()
        m.ParseFromString(body)
        assert m.Results[0].Type == 12
        t = m.Results[0].SortedColumns
        assert list(t.Columns) == wc[:3].tolist() and list(t.Values) == wv[:3].tolist() and not t.Keys
        got = c.query_node(srv.node, "i", "Sort(Row(f=1), field=v, sort-desc=true)", None)[0]
        assert isinstance(got, SortedColumns) and got == SortedColumns(wc, wv)
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
        mask = np.isin(cols, in_f)
        assert mask.sum() > 125
        for desc in (False, True):
            wc, wv = _small_oracle(cols, vals, mask, desc)
            for off, lim in WINDOWS:
                q = call_text("v", "Row(f=1)", limit=lim, offset=off, desc=desc)
                one = c.query(single[0].uri, "i", q)["results"][0]
                hi = None if lim is None else (off or 0) + lim
                assert one == {"columns": wc[off or 0:hi].tolist(), "values": wv[off or 0:hi].tolist()}, q
                for s in servers:
                    assert c.query(s.uri, "i", q)["results"][0] == one, (q, s.node.id)
        # a page that holds entries of both nodes
        page = c.query(servers[0].uri, "i", call_text("v", "Row(f=1)", limit=50, offset=40))["results"][0]
        assert len({col // SW for col in page["columns"]}) > 1
    finally:
        _close(servers + single)


# ---------------------------------------------------------------- mesh
MESH_QUERIES = ["Sort(field=v)",
                "Sort(field=v, limit=50, offset=80)",
                "Sort(Row(f=1), field=v, sort-desc=true)",
                "Sort(Not(Row(g=3)), field=v, limit=40, offset=30, sort-desc=true)",
                "Sort(Row(f=1), field=v, offset=20)",
                "Sort(Row(g=9), field=v)"]


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
    cols = np.array(sorted(last), np.uint64)
    v = np.array([last[int(c)] for c in cols], np.int64)
    order = np.lexsort((cols, v))
    full, page = json.loads(want[0])[0], json.loads(want[1])[0]
    assert full == {"columns": cols[order].tolist(), "values": v[order].tolist()} and len(cols) > 400
    assert page == {"columns": full["columns"][80:130], "values": full["values"][80:130]}
    assert len({c // SW for c in page["columns"]}) > 1, "the page lies inside one shard"
    assert json.loads(want[5])[0] == {"columns": [], "values": []}
