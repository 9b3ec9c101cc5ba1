"""Extract(filter, Rows(field=)...): what the columns of a filter hold, on the
host path.  Pilosa v1.3 has no such call, so every answer is pinned to numpy
over the known values; all answers are exact."""
import datetime as dt
import json
import os
import tempfile

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import ExecOptions, ExtractedTable, SignedRow
from pilosa_amd.models.row import Row

from tests.distinct_util import load
from tests.extract_util import call_text, check_ints, filters, int_cells, window
from tests.helpers import SW, Env
from tests.test_distinct import SHARDS, Data

INT_FIELDS = ("v", "w", "big", "nb")   # +-, a base, depth 40, a negative base


def _load_set_like(env, d, seed=7):
    """st: rows 2, 5, 9 at random (a column holds 0..3 of them); tm: a time
    field, rows 1 and 3; mx: a mutex over half the columns; bl: a bool over a
    third; ks: a keyed set field."""
    rng = np.random.default_rng(seed)
    idx = env.holder.index("i")
    every = np.concatenate([d.cols, d.extra])
    n = len(every)
    env.field("i", "st")
    env.field("i", "tm", type="time", time_quantum="YMD")
    env.field("i", "mx", type="mutex")
    env.field("i", "bl", type="bool")
    env.field("i", "ks", keys=True)
    d.member = {}
    for name, rows in (("st", (2, 5, 9)), ("tm", (1, 3))):
        d.member[name] = {r: rng.random(n) < 0.4 for r in rows}
        for r, m in d.member[name].items():
            ts = [dt.datetime(2019, 3, 1 + r)] * int(m.sum()) if name == "tm" else None
            idx.field(name).import_bits(np.full(int(m.sum()), r, np.uint64), every[m], ts)
    d.mx_has = rng.random(n) < 0.5
    d.mx_row = rng.integers(0, 6, n).astype(np.uint64)
    idx.field("mx").import_bits(d.mx_row[d.mx_has], every[d.mx_has])
    d.bl_has = rng.random(n) < 0.33
    d.bl_val = rng.random(n) < 0.5
    idx.field("bl").import_bits(d.bl_val[d.bl_has].astype(np.uint64), every[d.bl_has])
    d.every = every
    d.ks_cols = every[:7]
    env.q("i", " ".join(f'Set({int(c)}, ks="{"ab"[k % 2]}")' for k, c in enumerate(d.ks_cols))
          + f' Set({int(d.ks_cols[0])}, ks="zz")')


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data()
    load(e, e.data)
    _load_set_like(e, e.data)
    yield e
    e.close()


def _at(d, columns):
    """Positions of ``columns`` in d.every."""
    order = np.argsort(d.every)
    return order[np.searchsorted(d.every[order], columns)]


def test_fixture(env):
    d = env.data
    g = {n: env.holder.field("i", n).bsi_group(n) for n in INT_FIELDS}
    assert g["big"].bit_depth == 40 and g["w"].base == 100 and g["nb"].base == -50
    assert (d.vals["v"] < 0).any() and (d.vals["v"] > 0).any() and not d.has["w"].all()
    fl = dict(filters(d))
    assert len(fl["Row(f=5)"]) == 1 and len(fl["Row(f=9)"]) == 0
    assert np.isin(d.extra, fl["Row(f=1)"]).all()
    assert sorted(set((d.cols // np.uint64(SW)).tolist())) == list(SHARDS)


@pytest.mark.parametrize("fields", [("v",), ("w",), ("big",), ("nb",), ("v", "w", "big", "nb")])
def test_int_fields_match_numpy(env, fields):
    d = env.data
    fl = filters(d, other="v" if "w" in fields else "w", bound=10 if "w" in fields else 500)
    assert len(fl) == 7
    for filt, columns in fl:
        got = env.q1("i", call_text(filt, fields))
        assert isinstance(got, ExtractedTable) and got.keys is None
        check_ints(d, got, fields, columns)


def test_columns_without_a_value_keep_their_place(env):
    d = env.data
    got = env.q1("i", call_text("Row(f=1)", ("v", "w")))
    at = np.isin(got.columns, d.extra)
    assert at.sum() == len(d.extra) == 3
    for i in range(2):
        assert not got.data[i][1][at].any()
    # w lacks every 5th column: the neighbours of a null keep their own values
    cells = got.cells(1)
    assert None in cells and cells == int_cells(d, "w", got.columns)


def test_set_like_fields_match_numpy(env):
    d = env.data
    got = env.q1("i", "Extract(Row(f=1), Rows(field=st), Rows(tm), Rows(field=mx), Rows(field=bl), Rows(field=v))")
    assert got.fields == [("st", "[]uint64"), ("tm", "[]uint64"), ("mx", "uint64"), ("bl", "bool"), ("v", "int64")]
    at = _at(d, got.columns)
    for i, name in ((0, "st"), (1, "tm")):
        want = [[r for r, m in sorted(d.member[name].items()) if m[p]] for p in at]
        assert got.cells(i) == want
        offs, rows = got.data[i]
        assert offs.dtype == np.int64 and rows.dtype == np.uint64 and len(offs) == len(got) + 1
        assert [] in want and any(len(x) > 1 for x in want)
    assert got.cells(2) == [int(d.mx_row[p]) if d.mx_has[p] else None for p in at]
    assert got.cells(3) == [bool(d.bl_val[p]) if d.bl_has[p] else None for p in at]
    assert {None, True, False} <= set(got.cells(3)) and None in got.cells(2)
    assert got.cells(4) == int_cells(d, "v", got.columns)


def test_keyed_field(env):
    d = env.data
    got = env.q1("i", "Extract(Row(f=1), Rows(field=ks), limit=40)")
    assert got.fields == [("ks", "[]string")]
    want = {int(c): (["a", "zz"] if k == 0 else ["ab"[k % 2]]) for k, c in enumerate(d.ks_cols)}
    assert got.cells(0) == [want.get(int(c), []) for c in got.columns]
    assert any(got.cells(0))
    js = json.loads(_json(got))
    assert js["fields"] == [{"name": "ks", "type": "[]string"}]
    assert [c["rows"][0] for c in js["columns"]] == got.cells(0)


def test_empty_filter_and_missing_views(env):
    for q in ("Extract(Row(f=9), Rows(field=v), Rows(field=st))",
              "Extract(Intersect(Row(f=2), Row(f=3)), Rows(field=v), Rows(field=st))",
              "Options(Extract(Row(f=1), Rows(field=v), Rows(field=st)), shards=[2])"):
        got = env.q1("i", q)
        assert got.fields == [("v", "int64"), ("st", "[]uint64")] and len(got) == 0
        assert got.data[1][0].tolist() == [0]
        assert json.loads(_json(got)) == {
            "fields": [{"name": "v", "type": "int64"}, {"name": "st", "type": "[]uint64"}], "columns": []}
    if env.holder.field("i", "unset") is None:
        env.field("i", "unset", type="int", min=0, max=10)      # no BSI view yet
    if env.holder.field("i", "unset_s") is None:
        env.field("i", "unset_s")
    got = env.q1("i", "Extract(Row(f=5), Rows(field=unset), Rows(field=unset_s), Rows(field=v))")
    assert len(got) == 1 and got.cells(0) == [None] and got.cells(1) == [[]] and got.cells(2)[0] is not None


def test_limit_and_offset_windows(env):
    d = env.data
    columns = dict(filters(d))["Row(f=1)"]
    per = [int((columns // np.uint64(SW) == s).sum()) for s in SHARDS]
    n = len(columns)
    assert all(p > 10 for p in per)
    cases = [(0, 5), (3, 5), (0, per[0]), (per[0], per[1]), (per[0] - 2, 4), (per[0] + per[1], 3),
             (per[0] + per[1] + 1, None), (n - 2, 10), (n, 5), (n + 7, None), (0, 0), (5, None), (0, n)]
    for off, lim in cases:
        got = env.q1("i", call_text("Row(f=1)", ("v", "st"), offset=off, limit=lim))
        want = window(columns, off, lim)
        check_ints(d, got, ("v",), want)
        full = env.q1("i", call_text("Row(f=1)", ("st",)))
        lo = min(off, n)
        assert got.cells(1) == full.cells(0)[lo:lo + len(want)], (off, lim)


def test_options_shards_and_remote_keeps_the_offset(env):
    d = env.data
    columns = dict(filters(d))["Row(f=1)"]
    sub = columns[np.isin(columns // np.uint64(SW), np.array([1, 3], np.uint64))]
    check_ints(d, env.q1("i", "Options(Extract(Row(f=1), Rows(field=v)), shards=[1, 3])"), ("v",), sub)
    # a node answering a remote request returns its first offset + limit columns
    got = env.executor.execute("i", call_text("Row(f=1)", ("v",), offset=4, limit=3),
                               opt=ExecOptions(remote=True)).results[0]
    check_ints(d, got, ("v",), columns[:7])


@pytest.mark.parametrize("q,msg", [
    ("Extract(Rows(field=v))", "Extract(): filter required"),
    ("Extract()", "Extract(): filter required"),
    ("Extract(Row(f=1), Row(f=2), Rows(field=v))", "Extract() only accepts a single bitmap input"),
    ("Extract(Row(f=1))", "Extract(): at least one Rows(field=) required"),
    ("Extract(Row(f=1), Rows(field=v, limit=3))", "Extract(): Rows() accepts only a field"),
    ("Extract(Row(f=1), Rows(field=v, previous=3))", "Extract(): Rows() accepts only a field"),
    ("Extract(Row(f=1), Rows(field=nope))", "field not found"),
    ("Extract(Row(f=1), Rows(field=v), Rows(v))", 'Extract(): duplicate field "v"'),
    ("Extract(Row(f=1), Rows(field=v), limit=-1)", "Extract(): limit must be a non-negative integer"),
    ('Extract(Row(f=1), Rows(field=v), limit="x")', "Extract(): limit must be a non-negative integer"),
    ("Extract(Row(f=1), Rows(field=v), offset=-2)", "Extract(): offset must be a non-negative integer"),
    ("Extract(Row(f=1), Rows(field=v), offset=true)", "Extract(): offset must be a non-negative integer"),
    ("Extract(Row(f=1), Rows(field=v), k=3)", 'Extract(): unknown argument "k"'),
    ("Extract(Row(f=1), Rows(field=v), field=v)", 'Extract(): unknown argument "field"'),
])
def test_errors(env, q, msg):
    with pytest.raises(PilosaError) as e:
        env.q("i", q)
    assert str(e.value) == msg


def test_field_not_found_is_worded_as_distinct_words_it(env):
    errs = []
    for q in ("Distinct(field=nope)", "Extract(Row(f=1), Rows(field=nope))"):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        errs.append(str(e.value))
    assert errs[0] == errs[1]


def test_nested_use_keeps_the_unknown_call_error(env):
    errs = []
    for q in ("Count(Extract(Row(f=1), Rows(field=v)))", "Count(NoSuchCall(Row(f=1), Rows(field=v)))"):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        errs.append(str(e.value).replace("NoSuchCall", "Extract"))
    assert errs[0] == errs[1]


def test_size_guard(env, monkeypatch):
    d = env.data
    columns = dict(filters(d))["Row(f=1)"]
    monkeypatch.setenv("PILOSA_EXTRACT_MAX_COLUMNS", "10")
    gathered = []
    import pilosa_amd.executor as X
    real = X.extract_field_shard
    monkeypatch.setattr(X, "extract_field_shard", lambda *a: gathered.append(1) or real(*a))
    for q, n in ((call_text("Row(f=1)", ("v",)), len(columns)),
                 (call_text("Row(f=1)", ("v",), offset=8, limit=3), 11),
                 (call_text("Row(f=5)", ("v",), offset=11, limit=0), 11)):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        assert str(e.value) == f"Extract(): {n} columns exceed the limit of 10; page with limit= and offset="
    assert not gathered, "the guard ran after values were gathered"
    check_ints(d, env.q1("i", call_text("Row(f=1)", ("v",), offset=7, limit=3)), ("v",), columns[7:10])
    check_ints(d, env.q1("i", call_text("Row(f=5)", ("v",))), ("v",), dict(filters(d))["Row(f=5)"])
    assert gathered


def _json(r) -> bytes:
    from pilosa_amd.server import encoding
    return encoding.result_json_bytes(r)


def _sample():
    return ExtractedTable(
        [("v", "int64"), ("s", "[]uint64"), ("m", "uint64"), ("b", "bool")], np.array([1, 5, SW + 2], np.uint64),
        [(np.array([-7, 0, 9], np.int64), np.array([True, False, True])),
         (np.array([0, 2, 3, 3], np.int64), np.array([1, 3, 1], np.uint64)),
         (np.array([0, 4, 0], np.uint64), np.array([False, True, False])),
         (np.array([True, False, False]), np.array([True, True, False]))])


def test_json_bytes():
    assert _json(_sample()) == (
        b'{"fields":[{"name":"v","type":"int64"},{"name":"s","type":"[]uint64"},{"name":"m","type":"uint64"},'
        b'{"name":"b","type":"bool"}],"columns":[{"column":1,"rows":[-7,[1,3],null,true]},'
        b'{"column":5,"rows":[null,[1],4,false]},{"column":%d,"rows":[9,[],null,null]}]}' % (SW + 2))
    assert _json(ExtractedTable([("v", "int64")])) == b'{"fields":[{"name":"v","type":"int64"}],"columns":[]}'


def test_equality_and_repr():
    a, b = _sample(), _sample()
    assert a == b and not (a != b) and a != SignedRow() and a != _sample().slice(0, 2)
    b.data[0][0][0] = 8
    assert a != b
    assert repr(a) == ("ExtractedTable(fields=[('v', 'int64'), ('s', '[]uint64'), ('m', 'uint64'), ('b', 'bool')], "
                       "columns=3)")
    assert a.slice(1, 3).cells(1) == [[1], []] and a.slice(1).columns.tolist() == [5, SW + 2]
    rev = a.take(np.array([2, 0, 1]))
    assert rev.cells(1) == [[], [1, 3], [1]] and rev.cells(0) == [9, -7, None]
    assert ExtractedTable.concat([a.slice(2), a.slice(0, 2)]) == a      # re-sorted by column


def test_protobuf_round_trip_and_type_code():
    from pilosa_amd import wire
    from pilosa_amd.executor import QueryResponse
    from pilosa_amd.server import encoding
    assert wire.QUERY_RESULT_TYPE_EXTRACTEDTABLE == 11
    keyed = ExtractedTable([("m", "string"), ("s", "[]string")], np.array([3, 4], np.uint64),
                           [(["x", ""], np.array([True, False])), (np.array([0, 0, 2], np.int64), ["p", "q"])],
                           keys=["c3", "c4"])
    for r in (_sample(), ExtractedTable([("v", "int64"), ("s", "[]uint64")]), keyed):
        m = encoding.result_to_pb(r, "Extract")
        assert m.Type == 11
        back = encoding.result_from_pb(wire.pb.QueryResult.FromString(m.SerializeToString()))
        assert isinstance(back, ExtractedTable) and back == r
    m = encoding.result_to_pb(_sample(), "Extract").ExtractedTable
    assert list(m.Columns) == [1, 5, SW + 2] and len(m.Fields) == 4
    # column-major: one sub-message per field, packed values, a validity bitmap, packed offsets
    assert list(m.Fields[0].Values) == [-7, 0, 9] and m.Fields[0].Valid == bytes([0b101])
    assert list(m.Fields[1].Offsets) == [0, 2, 3, 3] and list(m.Fields[1].Rows) == [1, 3, 1]
    assert list(m.Fields[2].Rows) == [0, 4, 0] and m.Fields[2].Valid == bytes([0b010])
    assert list(m.Fields[3].Values) == [1, 0, 0] and m.Fields[3].Valid == bytes([0b011])
    # ExtractedTable = 11 (0x5a), Type = 6 (0x30)
    raw = encoding.result_to_pb(ExtractedTable([("v", "int64")], np.array([3], np.uint64),
                                               [(np.array([4], np.int64), np.array([True]))]),
                                "Extract").SerializeToString()
    assert raw == bytes.fromhex("300b" "5a15" "0a10""0a0176" "1205696e743634" "1a0104" "320101" "120103")
    resp = encoding.response_from_pb(encoding.response_to_pb(QueryResponse([_sample(), 3])))
    assert resp.results[0] == _sample() and resp.results[1] == 3


def test_a_million_columns_encode_without_a_loop_per_cell():
    """Column-major encoding: the work per cell is inside numpy and protobuf,
    so a 2^20-column table encodes in a handful of Python-level calls."""
    import sys
    from pilosa_amd.server import encoding
    n = 1 << 20
    t = ExtractedTable([("v", "int64")], np.arange(n, dtype=np.uint64),
                       [(np.arange(n, dtype=np.int64), np.ones(n, bool))])
    calls = [0]

    def count(frame, event, arg):
        calls[0] += event == "call"
    sys.setprofile(count)
    try:
        m = encoding.result_to_pb(t, "Extract")
    finally:
        sys.setprofile(None)
    assert calls[0] < 100 and len(m.ExtractedTable.Fields[0].Values) == n


def test_existing_results_keep_their_bytes():
    """Golden bytes written out by hand from the proto: QueryResult{Row = 1,
    SignedRow = 10, Type = 6}."""
    from pilosa_amd.server import encoding
    row = encoding.result_to_pb(Row([1, 5, 300]), "Row").SerializeToString()
    assert row == bytes.fromhex("0a06" "0a04" "0105ac02" "3001")
    sr = encoding.result_to_pb(SignedRow(Row([3]), Row([4])), "Distinct").SerializeToString()
    assert sr == bytes.fromhex("300a520a0a030a010412030a0103")
    assert encoding.result_json_bytes(Row([1, 5, 300])) == b'{"attrs":{},"columns":[1,5,300]}'
    assert encoding.result_json_bytes(SignedRow(Row([3]), Row([4]))) == \
        b'{"pos":{"attrs":{},"columns":[3]},"neg":{"attrs":{},"columns":[4]}}'


def test_partial_round_trip():
    from pilosa_amd.parallel.collectives import TAG_EXTRACT, TAG_ROW, decode_partial, encode_partial
    assert TAG_EXTRACT == 13
    big = ExtractedTable([("u", "uint64")], np.array([1 << 40], np.uint64),
                         [(np.array([(1 << 64) - 1], np.uint64), np.array([True]))])
    for r in (_sample(), ExtractedTable([("v", "int64"), ("s", "[]uint64")]), big):
        w = encode_partial(r)
        assert w.dtype == np.int64 and int(w[0]) == TAG_EXTRACT
        back = decode_partial(w)
        assert isinstance(back, ExtractedTable) and back == r
        for (a, b), (c, d) in zip(back.data, r.data):
            assert a.dtype == c.dtype and b.dtype == d.dtype
    row = Row([1, SW + 7])
    w = encode_partial(row)
    assert int(w[0]) == TAG_ROW and decode_partial(w) == row


def test_parsers_agree():
    from pilosa_amd import _pql
    from pilosa_amd.pql import Call
    from pilosa_amd.pql import parser as P
    assert P._native is _pql, "parse_string does not use the native parser"
    text = "Extract(Intersect(Row(g=1), Not(Row(h=2))), Rows(field=v), Rows(w), limit=10, offset=3)"
    a, b = _pql.parse_calls(text), P.parse_string_py(text).calls
    want = Call("Extract", {"limit": 10, "offset": 3},
                [Call("Intersect", {}, [Call("Row", {"g": 1}), Call("Not", {}, [Call("Row", {"h": 2})])]),
                 Call("Rows", {"field": "v"}), Call("Rows", {"_field": "w"})])
    assert list(a) == b == [want] == P.parse_string(text).calls
    for text in ("Extract(Row(f=1), Rows(field=v))", "Extract(Row(v > 10), Rows(w), Rows(field=v), limit=2)"):
        c = P.parse_string(text).calls[0]
        assert P.parse_string(str(c)).calls[0] == c == P.parse_string_py(str(c)).calls[0], str(c)


def test_keyed_index_and_column_attrs():
    e = Env()
    try:
        e.create_index("k", keys=True)
        e.field("k", "f", keys=True)
        e.field("k", "m", type="mutex", keys=True)
        e.field("k", "v", type="int", min=-100, max=100)
        vals = {"a": 7, "b": -7, "c": 0, "d": 7}
        e.q("k", " ".join(f'Set("{c}", v={x})' for c, x in vals.items()) +
            ' Set("a", f="x") Set("b", f="x") Set("e", f="x") Set("b", f="y") Set("a", m="one") Set("e", m="two")')
        got = e.q1("k", 'Extract(Row(f="x"), Rows(field=v), Rows(field=f), Rows(field=m))')
        assert got.fields == [("v", "int64"), ("f", "[]string"), ("m", "string")]
        assert got.keys == ["a", "b", "e"]
        assert got.cells(0) == [7, -7, None] and got.cells(1) == [["x"], ["x", "y"], ["x"]]
        assert got.cells(2) == ["one", None, "two"]
        assert json.loads(_json(got))["columns"] == [
            {"column": "a", "rows": [7, ["x"], "one"]}, {"column": "b", "rows": [-7, ["x", "y"], None]},
            {"column": "e", "rows": [None, ["x"], "two"]}]
        assert e.q1("k", 'Extract(Row(f="x"), Rows(field=v), limit=1, offset=1)').keys == ["b"]
        e.q("k", " ".join(f'SetColumnAttrs("{c}", tag="t{c}")' for c in vals))
        resp = e.executor.execute("k", 'Options(Row(f="x"), columnAttrs=true)')
        assert resp.column_attr_sets, "the fixture's columns carry no attributes"
        resp = e.executor.execute("k", 'Options(Extract(Row(f="x"), Rows(field=v)), columnAttrs=true)')
        assert not resp.column_attr_sets and resp.results[0].cells(0) == [7, -7, None]
    finally:
        e.close()


# ---------------------------------------------------------------- servers
WINDOWS = [(None, None), (0, 7), (5, 40), (120, 50), (140, None)]


def test_http_json_and_protobuf_results():
    from pilosa_amd.wire import pb
    from tests.test_percentile import _close, _load_small, _req, _servers
    servers = _servers(1)
    try:
        srv = servers[0]
        c, cols, vals, in_f = _load_small(servers)
        val = dict(zip(cols.tolist(), vals.tolist()))
        want = [{"column": int(x), "rows": [val[int(x)]]} for x in np.sort(in_f)]
        body = _req(srv, "/index/i/query", b"Extract(Row(f=1), Rows(field=v))")
        assert json.loads(body) == {"results": [{"fields": [{"name": "v", "type": "int64"}], "columns": want}]}
        body = _req(srv, "/index/i/query",
                    pb.QueryRequest(Query="Extract(Row(f=1), Rows(field=v), limit=3)").SerializeToString(),
                    {"Content-Type": "application/x-protobuf", "Accept": "application/x-protobuf"})
        m = pb.QueryResponse()
        m.ParseFromString(body)
        assert m.Results[0].Type == 11
        t = m.Results[0].ExtractedTable
        assert list(t.Columns) == [w["column"] for w in want[:3]]
        assert list(t.Fields[0].Values) == [w["rows"][0] for w in want[:3]]
        got = c.query_node(srv.node, "i", "Extract(Row(f=1), Rows(field=v))", None)[0]
        assert isinstance(got, ExtractedTable) and got.cells(0) == [w["rows"][0] for w in want]
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
        val = dict(zip(cols.tolist(), vals.tolist()))
        every = np.sort(in_f)
        assert len(every) > 125
        for off, lim in WINDOWS:
            q = call_text("Row(f=1)", ("v", "f"), offset=off, limit=lim)
            one = c.query(single[0].uri, "i", q)["results"][0]
            assert one["columns"] == [{"column": int(x), "rows": [val[int(x)], [1]]}
                                      for x in window(every, off or 0, lim)], q
            for s in servers:
                assert c.query(s.uri, "i", q)["results"][0] == one, (q, s.node.id)
    finally:
        _close(servers + single)


# ---------------------------------------------------------------- mesh
MESH_QUERIES = ["Extract(Row(f=1), Rows(field=v), Rows(field=g))",
                "Extract(Row(f=1), Rows(field=v), Rows(field=g), limit=50, offset=80)",
                "Extract(Not(Row(g=3)), Rows(field=v), limit=400, offset=300)",
                "Extract(Row(f=2), Rows(field=g), offset=100)",
                "Extract(Row(g=9), Rows(field=v))"]


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
    full, page = json.loads(want[0])[0], json.loads(want[1])[0]
    f1 = sorted({col for fld, row, col in bits if fld == "f" and row == 1})
    assert [c["column"] for c in full["columns"]] == f1 and len(f1) > 130
    assert page["columns"] == full["columns"][80:130]
    assert len({c["column"] // SW for c in page["columns"]}) > 1, "the page lies inside one shard"
    assert json.loads(want[4])[0]["columns"] == []
