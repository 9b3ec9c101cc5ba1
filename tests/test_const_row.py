"""ConstRow(columns=[...]): a literal row given by its column ids, on the host
path.  Pilosa v1.3 has no such call (it was added later), so every answer is
pinned to numpy set arithmetic over the known columns, or to the same call
under a stored row that holds exactly the listed columns."""
import json
import os
import tempfile

import numpy as np
import pytest

from pilosa_amd.errors import BadRequestError, PilosaError
from pilosa_amd.executor import ExecOptions, const_row_columns
from pilosa_amd.models.row import Row
from pilosa_amd.pql import Call, Query

from tests.const_row_util import row_of, text
from tests.distinct_util import load
from tests.extract_util import check_ints
from tests.helpers import SW, Env, cols
from tests.sort_util import check, oracle
from tests.test_distinct import SHARDS, Data

STORED = 7   # row of f that holds exactly the columns of LIST_A inside the shards


class Lists:
    """The column lists of the tests over tests/test_distinct.py's fixture
    (shards 0, 1, 3): ``a`` -- unsorted, with duplicates, with columns the
    existence field lacks (``ghosts``), with columns of shard 2 (absent) and
    shard 9 (never requested), and the last column of shard 0 next to the
    first of shard 1; ``b`` -- every third valued column."""

    def __init__(self, d):
        rng = np.random.default_rng(11)
        known = set(d.cols.tolist()) | set(d.extra.tolist())
        self.ghosts = [c for c in (6, SW - 1, SW, SW + 77, 3 * SW + 4000) if c not in known]
        assert len(self.ghosts) == 5
        self.outside = [2 * SW + 5, 2 * SW + SW - 1, 9 * SW + 1]
        picked = d.cols[rng.random(len(d.cols)) < 0.3].tolist()
        a = picked + self.ghosts + self.outside + picked[:40] + [int(d.extra[0])]
        self.a = [a[i] for i in rng.permutation(len(a))]
        self.b = d.cols[::3].tolist()
        assert self.a != sorted(self.a) and len(set(self.a)) < len(self.a)


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data()
    load(e, e.data)
    e.lists = Lists(e.data)
    inside = np.array(row_of(e.lists.a, SHARDS), np.uint64)
    e.holder.index("i").field("f").import_bits(np.full(len(inside), STORED, np.uint64), inside)
    yield e
    e.close()


def _f1(d):
    return set(d.cols[d.rows[1]].tolist()) | set(d.extra.tolist())


# ---------------------------------------------------------------- algebra
def test_alone_is_the_listed_columns_inside_the_requested_shards(env):
    L = env.lists
    want = row_of(L.a, SHARDS)
    got = env.q1("i", text(L.a))
    assert isinstance(got, Row) and got.attrs in (None, {}) and cols(got) == want
    assert set(L.ghosts) <= set(want) and not set(L.outside) & set(want)
    assert env.q1("i", f"Count({text(L.a)})") == len(want)
    # order and duplicates do not matter
    assert cols(env.q1("i", text(sorted(set(L.a))))) == want
    # the shards of the request decide, not the list
    assert cols(env.q1("i", f"Options({text(L.a)}, shards=[1, 9])")) == row_of(L.a, (1, 9))
    assert 9 * SW + 1 in row_of(L.a, (1, 9))
    assert cols(env.q1("i", text(L.outside))) == []
    assert cols(env.q1("i", text([2 ** 63 - 1, 0]))) == [0]


def test_set_operations_match_numpy(env):
    d, L = env.data, env.lists
    a, b, f1 = set(row_of(L.a, SHARDS)), set(row_of(L.b, SHARDS)), _f1(d)
    ta, tb = text(L.a), text(L.b)
    for q, want in ((f"Intersect({ta}, {tb})", a & b),
                    (f"Intersect(Row(f=1), {ta})", f1 & a),
                    (f"Union({ta}, {tb})", a | b),
                    (f"Union(Row(f=1), {ta})", f1 | a),
                    (f"Difference({ta}, {tb})", a - b),
                    (f"Difference(Row(f=1), {ta})", f1 - a),
                    (f"Difference({ta}, Row(f=1))", a - f1),
                    (f"Xor({ta}, {tb})", a ^ b),
                    (f"Xor({ta}, Row(f=1), {tb})", a ^ f1 ^ b),
                    (f"Shift({ta}, n=1)", {c + 1 for c in a}),
                    (f"Intersect(Shift({ta}, n=1), {tb})", {c + 1 for c in a} & b),
                    (f"Union(Intersect({ta}, {tb}), Difference(Row(f=4), {ta}))",
                     (a & b) | (set(d.cols[d.rows[4]].tolist()) - a))):
        assert cols(env.q1("i", q)) == sorted(want), q[:40]
        assert env.q1("i", f"Count({q})") == len(want), q[:40]
    assert SW - 1 in a and SW in {c + 1 for c in a}, "no bit shifts across a shard boundary"


def test_existence_is_not_consulted(env):
    d, L = env.data, env.lists
    exists = set(d.cols.tolist()) | set(d.extra.tolist())
    a = set(row_of(L.a, SHARDS))
    assert cols(env.q1("i", text(L.ghosts))) == sorted(L.ghosts)
    assert env.q1("i", f"Count({text(L.ghosts)})") == len(L.ghosts)
    assert cols(env.q1("i", f"Not({text(L.a)})")) == sorted(exists - a)
    assert cols(env.q1("i", f"Not(Not({text(L.a)}))")) == sorted(exists & a)     # the ghosts are gone
    assert cols(env.q1("i", f"Intersect(Row(f=1), {text(L.ghosts)})")) == []
    assert cols(env.q1("i", f"Intersect(Not(Row(f=9)), {text(L.ghosts)})")) == []


# ---------------------------------------------------------------- as a filter
def test_filter_of_every_consumer_equals_a_stored_row(env):
    d, L = env.data, env.lists
    ta, stored = text(L.a), f"Row(f={STORED})"
    assert cols(env.q1("i", stored)) == row_of(L.a, SHARDS)
    for shape in ("Sum({}, field=v)", "Min({}, field=v)", "Max({}, field=w)", "Percentile({}, field=v, nth=50)",
                  "Percentile({}, field=w, nth=99.9)", "Distinct({}, field=v)", "Distinct({}, field=nb)",
                  "TopK({}, field=f, k=3)", "TopK({}, field=f)", "TopN(f, {}, n=3)", "TopN(f, {})",
                  "Sort({}, field=v, limit=25, offset=3)", "Sort({}, field=s, sort-desc=true)",
                  "Extract({}, Rows(field=v), Rows(field=f), limit=30, offset=5)", "Extract({}, Rows(field=w))",
                  "GroupBy(Rows(field=f), filter={})", "GroupBy(Rows(field=f), filter={}, aggregate=Sum(field=v))",
                  "Count(Intersect({}, Row(v > 0)))"):
        got, want = env.q1("i", shape.format(ta)), env.q1("i", shape.format(stored))
        assert got == want, shape
        assert got not in (None, [], 0), shape


def test_filter_answers_match_numpy(env):
    d, L = env.data, env.lists
    mask = np.isin(d.cols, np.array(L.a, np.uint64))
    assert 100 < mask.sum() < len(d.cols)
    got = env.q1("i", f"Sum({text(L.a)}, field=v)")
    assert (got.val, got.count) == (int(d.vals["v"][mask].sum()), int(mask.sum()))
    check(env.q1("i", f"Sort({text(L.a)}, field=v, sort-desc=true)"), oracle(d, "v", mask, True))
    listed = np.array(row_of(L.a, SHARDS), np.uint64)
    table = env.q1("i", f"Extract({text(L.a)}, Rows(field=v), Rows(field=w))")
    check_ints(d, table, ("v", "w"), listed)          # ghosts keep their place, valueless
    groups = {g.group[0].row_id: g.count for g in env.q1("i", f"GroupBy(Rows(field=f), filter={text(L.a)})")}
    assert groups[1] == int((d.rows[1] & mask).sum()) + 1 and groups[STORED] == len(listed)   # + extra[0]


# ---------------------------------------------------------------- errors
@pytest.mark.parametrize("q,msg", [
    ("ConstRow()", "ConstRow(): columns required"),
    ("ConstRow(columns=3)", "ConstRow(): columns must be a list of unsigned integers"),
    ("ConstRow(columns=[1, -2])", "ConstRow(): columns must be a list of unsigned integers"),
    ("ConstRow(columns=[1, 2.5])", "ConstRow(): columns must be a list of unsigned integers"),
    ("ConstRow(columns=null)", "ConstRow(): columns must be a list of unsigned integers"),
    ("ConstRow(Row(f=1), columns=[1])", "ConstRow() accepts no bitmap input"),
    ("ConstRow(columns=[1], limit=2)", 'ConstRow(): unknown argument "limit"'),
    ("ConstRow(column=[1])", 'ConstRow(): unknown argument "column"'),
])
def test_errors(env, q, msg):
    for shape in ("Count({})", "Sum({}, field=v)", "Count(Intersect(Row(f=1), {}))", "GroupBy(Rows(field=f), filter={})"):
        with pytest.raises(PilosaError) as e:
            env.q("i", shape.format(q))
        assert str(e.value) == msg, shape
    with pytest.raises(PilosaError) as e:      # a top-level bitmap call's errors come through the map step
        env.q("i", q)
    assert str(e.value).endswith(msg)


@pytest.mark.parametrize("value", [[True], [1, False], [1.0], 7, True, (1, 2), [np.uint64(3)], [1 << 63]])
def test_calls_built_in_code_are_checked_too(env, value):
    call = Call("Count", {}, [Call("ConstRow", {"columns": value})])
    with pytest.raises(PilosaError) as e:
        env.executor.execute("i", Query([call]))
    assert str(e.value) == "ConstRow(): columns must be a list of unsigned integers"


def test_an_empty_list_built_in_code_is_an_empty_row(env):
    assert cols(env.executor.execute("i", Query([Call("ConstRow", {"columns": []})])).results[0]) == []
    call = Call("Count", {}, [Call("Union", {}, [Call("ConstRow", {"columns": []}), Call("Row", {"f": 5})])])
    assert env.executor.execute("i", Query([call])).results[0] == 1
    from pilosa_amd.pql import ParseError, parse_string
    with pytest.raises(ParseError):          # both parsers reject [] as before
        parse_string("ConstRow(columns=[])")


def test_size_guard(env, monkeypatch):
    monkeypatch.setenv("PILOSA_CONSTROW_MAX_COLUMNS", "10")
    eleven = list(range(11))
    for shape in ("Count({})", "Extract({}, Rows(field=v))"):
        with pytest.raises(PilosaError) as e:
            env.q("i", shape.format(text(eleven)))
        assert str(e.value) == "ConstRow(): 11 columns exceed the limit of 10"
    with pytest.raises(PilosaError) as e:      # the list as written counts, duplicates included
        env.q("i", f"Count({text([3] * 11)})")
    assert str(e.value) == "ConstRow(): 11 columns exceed the limit of 10"
    assert env.q1("i", f"Count({text(eleven[:10])})") == 10
    monkeypatch.delenv("PILOSA_CONSTROW_MAX_COLUMNS")
    assert env.q1("i", f"Count({text(eleven)})") == 11
    big = Call("Count", {}, [Call("ConstRow", {"columns": [0] * ((1 << 20) + 1)})])
    with pytest.raises(PilosaError) as e:
        env.executor.execute("i", Query([big]))
    assert str(e.value) == f"ConstRow(): {(1 << 20) + 1} columns exceed the limit of {1 << 20}"


def test_the_list_is_sorted_once_per_call_object(env, monkeypatch):
    L = env.lists
    call = Call("ConstRow", {"columns": list(L.a)})
    first = const_row_columns(call)
    assert first.dtype == np.uint64 and first.tolist() == sorted(set(L.a))
    assert const_row_columns(call) is first
    real, n = np.unique, []
    monkeypatch.setattr(np, "unique", lambda *a, **k: n.append(1) or real(*a, **k))
    assert len(cols(env.executor.execute("i", Query([Call("ConstRow", {"columns": list(L.a)})])).results[0])) > 100
    assert len(n) == 1, "the list was sorted once per shard"
    # a clone and an equal call do not share or compare the memo
    assert call.clone() == call and call.clone().memo is None
    call.args["columns"] = [5, 4]
    assert const_row_columns(call).tolist() == [4, 5]


# ---------------------------------------------------------------- keys
def test_keyed_index():
    e = Env()
    try:
        e.create_index("k", keys=True)
        e.field("k", "f", keys=True)
        e.field("k", "v", type="int", min=-100, max=100)
        e.q("k", 'Set("a", f="x") Set("b", f="x") Set("c", f="y") Set("d", f="x") Set("a", v=4) Set("c", v=-9)')
        got = e.q1("k", 'ConstRow(columns=["c", "a", "a"])')
        assert isinstance(got, Row) and sorted(got.keys) == ["a", "c"]
        assert e.q1("k", 'Count(Intersect(Row(f="x"), ConstRow(columns=["a", "c", "d"])))') == 2
        assert e.q1("k", 'Sort(ConstRow(columns=["c", "a", "b"]), field=v)').keys == ["c", "a"]
        got = e.q1("k", 'Extract(ConstRow(columns=["c", "b"]), Rows(field=v), Rows(field=f))')
        assert sorted(zip(got.keys, got.cells(0), got.cells(1))) == [("b", None, ["x"]), ("c", -9, ["y"])]
        assert [g.count for g in e.q1("k", 'GroupBy(Rows(field=f), filter=ConstRow(columns=["a", "c"]))')] == [1, 1]
        for q in ("ConstRow(columns=[1])", 'Count(ConstRow(columns=["a", 2]))',
                  'GroupBy(Rows(field=f), filter=ConstRow(columns=[3]))'):
            with pytest.raises(BadRequestError) as err:
                e.q("k", q)
            assert str(err.value) == "column value must be a string when index 'keys' option enabled"
    finally:
        e.close()


def test_string_items_on_an_unkeyed_index(env):
    errs = []
    for q in ('Count(ConstRow(columns=["a"]))', 'ConstRow(columns=[1, "b"])', 'Count(Count(Row(f=1)), col="a")'):
        with pytest.raises(BadRequestError) as e:
            env.q("i", q)
        errs.append(str(e.value))
    assert errs[0] == errs[1] == errs[2] == "string 'col' value not allowed unless index 'keys' option enabled"


# ---------------------------------------------------------------- parsers, text, encodings
def test_parsers_agree_and_a_long_list_round_trips():
    from pilosa_amd import _pql
    from pilosa_amd.pql import parser as P
    assert P._native is _pql, "parse_string does not use the native parser"
    t = "Count(Intersect(Row(g=1), Not(ConstRow(columns=[7, 3, 9223372036854775807, 3]))))"
    want = Call("Count", {}, [Call("Intersect", {}, [
        Call("Row", {"g": 1}), Call("Not", {}, [Call("ConstRow", {"columns": [7, 3, 2 ** 63 - 1, 3]})])])])
    assert list(_pql.parse_calls(t)) == P.parse_string_py(t).calls == [want] == P.parse_string(t).calls
    assert str(want) == "Count(Intersect(Row(g=1), Not(ConstRow(columns=[7,3,9223372036854775807,3]))))"
    rng = np.random.default_rng(2)
    big = Call("Extract", {"limit": 100000}, [Call("ConstRow", {"columns": rng.integers(0, 1 << 40, 100000).tolist()}),
                                              Call("Rows", {"_field": "v"})])
    s = str(big)
    assert len(s) > 500000
    assert P.parse_string(s).calls == [big] == P.parse_string_py(s).calls
    assert str(P.parse_string(s).calls[0]) == s


def test_a_count_request_holding_a_const_row_leaves_the_native_subset(env):
    """Five Count calls, one with a ConstRow: the native compilers decline
    that text (the device executor then plans it), and the answers are right."""
    from pilosa_amd import _pql
    d, L = env.data, env.lists
    qs = ["Count(Row(f=1))", "Count(Intersect(Row(f=1), Row(f=4)))",
          f"Count(Intersect(Row(f=1), {text(L.b)}))", "Count(Union(Row(f=2), Row(f=3)))", "Count(Row(f=5))"]
    dirs = [np.arange(1, 8, dtype=np.uint64)]
    _, ok = _pql.compile_counts(qs, {"f": 0}, dirs)
    assert ok.tolist() == [True, True, False, True, True]
    assert _pql.plan_count_text(" ".join(qs), {"f": 0}, dirs, True, True, 1, {}) is None
    assert _pql.plan_count_text(" ".join(qs[:2] + qs[3:]), {"f": 0}, dirs, True, True, 1, {}) is not None
    from pilosa_amd.ops.planner import GpuPlanner, Unsupported
    from pilosa_amd.pql import parse_string
    with pytest.raises(Unsupported):
        GpuPlanner(lambda f, v: None).plan(parse_string(qs[2]).calls[0])
    f1 = _f1(d)
    assert env.q("i", " ".join(qs)) == [len(f1), int((d.rows[1] & d.rows[4]).sum()), len(f1 & set(L.b)),
                                        len(d.cols), 1]


def test_row_results_keep_their_bytes(env):
    from pilosa_amd.server import encoding
    got = env.q1("i", "ConstRow(columns=[300, 1, 5, 5])")
    assert encoding.result_to_pb(got, "ConstRow").SerializeToString() == bytes.fromhex("0a06" "0a04" "0105ac02" "3001")
    assert encoding.result_to_pb(Row([1, 5, 300]), "Row").SerializeToString() == \
        bytes.fromhex("0a06" "0a04" "0105ac02" "3001")
    assert encoding.result_json_bytes(got) == b'{"attrs":{},"columns":[1,5,300]}'
    from pilosa_amd.parallel.collectives import TAG_ROW, decode_partial, encode_partial
    w = encode_partial(got)
    assert int(w[0]) == TAG_ROW and decode_partial(w) == Row([1, 5, 300])


def test_remote_nodes_evaluate_the_call_as_text(env):
    L = env.lists
    r = env.executor.execute("i", f"Count({text(L.a)})", shards=[1], opt=ExecOptions(remote=True)).results[0]
    assert r == len(row_of(L.a, (1,)))


# ---------------------------------------------------------------- cluster
def test_two_node_cluster_matches_numpy():
    from tests.test_percentile import _close, _load_small, _servers
    servers = _servers(2)
    try:
        c, cs, vals, in_f = _load_small(servers)
        owners = {s.node.id: sorted(s.holder.field("i", "v").view("bsig_v").fragments) for s in servers}
        assert all(owners.values()), owners
        listed = cs[::2].tolist() + [2 * SW + 1, 7]          # + an absent shard, + a column nobody set
        t = text(listed[::-1] + listed[:9])
        inside = row_of(listed, SHARDS)
        mask = np.isin(cs, np.array(listed, np.uint64))
        for s in servers:
            assert c.query(s.uri, "i", t)["results"][0]["columns"] == inside
            assert c.query(s.uri, "i", f"Count(Intersect(Row(f=1), {t}))")["results"][0] == \
                len(set(in_f.tolist()) & set(listed))
            got = c.query(s.uri, "i", f"Sum({t}, field=v)")["results"][0]
            assert got == {"value": int(vals[mask].sum()), "count": int(mask.sum())}
            off = sum(col < SW for col in inside) - 10          # a page with columns of both nodes
            got = c.query(s.uri, "i", f"Extract({t}, Rows(field=v), limit=20, offset={off})")["results"][0]
            assert [x["column"] for x in got["columns"]] == inside[off:off + 20]
            assert len({col // SW for col in inside[off:off + 20]}) > 1, "the page lies inside one shard"
            want = dict(zip(cs.tolist(), vals.tolist()))
            assert [x["rows"][0] for x in got["columns"]] == [want.get(col) for col in inside[off:off + 20]]
    finally:
        _close(servers)


# ---------------------------------------------------------------- mesh
def _mesh_queries():
    from tests.test_mesh import _data
    bits, vals = _data()
    listed = sorted({col for _, _, col in bits[::3]} | {col for col, _ in vals[::2]})
    t = text(listed[::-1] + listed[:5] + [50 * SW + 3])
    off = sum(col < 3 * SW for col in listed) - 40               # a page with columns of two shards
    return [t, f"Count({t})", f"Count(Intersect(Row(f=1), {t}))", f"Not({t})", f"Union(Row(g=2), Shift({t}, n=3))",
            f"Sum({t}, field=v)", f"Sort({t}, field=v, limit=30, offset=10)",
            f"Extract({t}, Rows(field=v), Rows(field=f), limit=80, offset={off})",
            f"GroupBy(Rows(field=f), filter={t})", f"TopK({t}, field=g)",
            f"Count(Row(f=1)) Count(Difference(Row(f=2), {t})) Count(Row(g=1))"], listed, off


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
        got = [_canon(ex.execute("i", q).results) for q in _mesh_queries()[0]]
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
    from pilosa_amd.parallel.mesh import _ROW_CALLS
    from tests.helpers import free_port
    from tests.test_mesh import _canon, _data, _load, _setup_schema

    assert "ConstRow" in _ROW_CALLS
    mp.start_processes(_mesh_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    res = json.load(open(tmp_path / "mesh.json"))
    holder = Holder(tempfile.mkdtemp(prefix="mesh_ref_")).open()
    ex = Executor(holder)
    try:
        _setup_schema(holder)
        bits, vals = _data()
        _load(ex, bits, vals)
        queries, listed, off = _mesh_queries()
        want = [_canon(ex.execute("i", q).results) for q in queries]
    finally:
        ex.close()
        holder.close()
    for q, g, w in zip(queries, res["got"], want):
        assert g == w, q[:60]
    assert json.loads(want[0])[0]["columns"] == listed and len({c // SW for c in listed}) > 3
    assert json.loads(want[1])[0] == len(listed)
    page = json.loads(want[7])[0]["columns"]
    assert [x["column"] for x in page] == listed[off:off + 80]
    assert len({x["column"] // SW for x in page}) > 1, "the page lies inside one shard"
