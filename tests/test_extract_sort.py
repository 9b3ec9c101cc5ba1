"""Extract(Sort(...), Rows(field=)+, [limit=], [offset=]): the fields of the
columns a Sort returns, in its order, on the host path.  Every answer is
pinned to numpy: tests/sort_util.py's oracle (np.lexsort by value, then
column) cut by both windows, then a gather of the known cells."""
import json
import os
import tempfile

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import ExecOptions, ExtractedTable

from tests.const_row_util import cut, extract_sort_text
from tests.distinct_util import load
from tests.extract_util import int_cells
from tests.helpers import SW, Env
from tests.sort_util import call_text as sort_text, oracle, tie_group
from tests.test_distinct import SHARDS, Data
from tests.test_extract import _at, _load_set_like

ALL = ("v", "st", "tm", "mx", "bl", "w", "big", "nb")
TYPES = {"v": "int64", "w": "int64", "big": "int64", "nb": "int64", "s": "int64", "st": "[]uint64", "tm": "[]uint64",
         "mx": "uint64", "bl": "bool"}


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data()
    load(e, e.data)
    _load_set_like(e, e.data)
    yield e
    e.close()


def cells(d, field, columns):
    """The oracle's cell of ``field`` for each of ``columns``, in their order."""
    if TYPES[field] == "int64":
        return int_cells(d, field, columns)
    at = _at(d, columns)
    if field in ("st", "tm"):
        return [[r for r, m in sorted(d.member[field].items()) if m[p]] for p in at]
    if field == "mx":
        return [int(d.mx_row[p]) if d.mx_has[p] else None for p in at]
    return [bool(d.bl_val[p]) if d.bl_has[p] else None for p in at]


def check_table(d, got, fields, columns):
    assert isinstance(got, ExtractedTable) and got.keys is None
    assert got.columns.dtype == np.uint64 and got.columns.tolist() == columns.tolist()
    assert got.fields == [(f, TYPES[f]) for f in fields]
    for i, f in enumerate(fields):
        assert got.cells(i) == cells(d, f, columns), f
        a, b = got.data[i]
        if TYPES[f].startswith("[]"):
            assert a.dtype == np.int64 and len(a) == len(columns) + 1 and a[0] == 0 and a[-1] == len(b)
        else:
            assert len(a) == len(b) == len(columns) and not np.asarray(a)[~b].any(), "a null carries a value"


def test_fixture(env):
    d = env.data
    want = oracle(d, "v", d.rows[1])
    assert (np.diff(want[0].astype(np.int64)) < 0).any(), "the sorted order is the column order"
    assert len({int(c) // SW for c in want[0][:40]}) > 1
    lo, hi = tie_group(oracle(d, "s", d.rows[1])[1])
    assert hi - lo > 50


@pytest.mark.parametrize("field", ["v", "w", "big", "nb", "s"])
@pytest.mark.parametrize("desc", [False, True])
def test_every_field_type_matches_numpy(env, field, desc):
    d = env.data
    for filt, mask in (("Row(f=1)", d.rows[1]), ("", np.ones(len(d.cols), bool)), ("Not(Row(f=4))", ~d.rows[4])):
        oc = oracle(d, field, mask, desc)[0][:60]
        fields = tuple(f for f in ALL if f != field)[:5] + (field,)            # the sort field itself, last
        q = extract_sort_text(sort_text(field, filt, limit=60, desc=desc if desc else None), fields)
        check_table(d, env.q1("i", q), fields, oc)
    # the sort field appears only if named
    got = env.q1("i", extract_sort_text(sort_text(field, "Row(f=1)", limit=5, desc=desc), ("mx",)))
    assert got.fields == [("mx", "uint64")]


def test_without_a_sort_limit_the_whole_answer_is_extracted(env):
    d = env.data
    oc = oracle(d, "w", d.rows[1])[0]
    assert len(oc) < int(d.rows[1].sum())          # w lacks values: those columns are not considered
    check_table(d, env.q1("i", extract_sort_text(sort_text("w", "Row(f=1)"), ("w", "st"))), ("w", "st"), oc)


def test_both_windows_combine(env):
    d = env.data
    for desc in (False, True):
        full = oracle(d, "v", d.rows[1], desc)[0]
        n = len(full)
        for s_off, s_lim in ((None, None), (0, 50), (7, 50), (n - 5, 50), (n, 3), (3, 0)):
            inner = cut(full, s_off or 0, s_lim)
            for e_off, e_lim in ((None, None), (0, 10), (5, 10), (45, 10), (49, None), (50, 4), (0, 0), (2, 0)):
                q = extract_sort_text(sort_text("v", "Row(f=1)", limit=s_lim, offset=s_off, desc=desc),
                                      ("v", "mx"), offset=e_off, limit=e_lim)
                check_table(d, env.q1("i", q), ("v", "mx"), cut(inner, e_off or 0, e_lim))


@pytest.mark.parametrize("desc", [False, True])
def test_cuts_inside_a_tie_group(env, desc):
    d = env.data
    full, vals = oracle(d, "s", d.rows[1], desc)
    lo, hi = tie_group(vals)
    assert len({int(c) // SW for c in full[lo:hi]}) > 1, "the tie group lies in one shard"
    for lim in (lo, lo + 1, (lo + hi) // 2, hi - 1, hi, hi + 1):
        q = extract_sort_text(sort_text("s", "Row(f=1)", limit=lim, desc=desc), ("s", "bl"))
        check_table(d, env.q1("i", q), ("s", "bl"), full[:lim])
    # Sort's window ends inside the group, Extract's starts inside it
    q = extract_sort_text(sort_text("s", "Row(f=1)", limit=hi - 2, desc=desc), ("s", "tm"), offset=lo + 3, limit=hi)
    check_table(d, env.q1("i", q), ("s", "tm"), full[:hi - 2][lo + 3:])
    # Sort's offset inside the group
    q = extract_sort_text(sort_text("s", "Row(f=1)", offset=lo + 2, limit=9, desc=desc), ("s",), limit=4, offset=1)
    check_table(d, env.q1("i", q), ("s",), full[lo + 2:lo + 11][1:5])


def test_empty_answers_are_header_only(env, monkeypatch):
    second = []
    real = type(env.executor).bitmap_call_shard
    monkeypatch.setattr(type(env.executor), "bitmap_call_shard",
                        lambda self, i, c, s: second.append(c.name) or real(self, i, c, s))
    for q in (extract_sort_text(sort_text("v", "Row(f=9)"), ("v", "st")),
              extract_sort_text(sort_text("v", "Intersect(Row(f=2), Row(f=3))", limit=5), ("v", "st")),
              extract_sort_text(sort_text("v", "Row(f=1)", limit=0), ("v", "st")),
              extract_sort_text(sort_text("v", "Row(f=1)", limit=9), ("v", "st"), limit=0),
              extract_sort_text(sort_text("v", "Row(f=1)", limit=9), ("v", "st"), offset=9),
              "Options(" + extract_sort_text(sort_text("v", "Row(f=1)"), ("v", "st")) + ", shards=[2])"):
        got = env.q1("i", q)
        assert got == ExtractedTable([("v", "int64"), ("st", "[]uint64")]) and len(got) == 0, q
    assert "ConstRow" not in second, "an empty answer ran the second phase"
    env.q1("i", extract_sort_text(sort_text("v", "Row(f=1)", limit=3), ("v",)))
    assert "ConstRow" in second


def test_options_shards(env):
    d = env.data
    mask = d.rows[1] & (d.cols // np.uint64(SW) != np.uint64(0))
    q = "Options(" + extract_sort_text(sort_text("v", "Row(f=1)", limit=30), ("v", "st"), offset=4) + ", shards=[1, 3])"
    check_table(d, env.q1("i", q), ("v", "st"), oracle(d, "v", mask)[0][:30][4:])


# ---------------------------------------------------------------- guards and errors
def test_a_large_filter_with_a_small_sort_limit_passes_the_extract_guard(env, monkeypatch):
    d = env.data
    monkeypatch.setenv("PILOSA_EXTRACT_MAX_COLUMNS", "10")
    assert int(d.rows[1].sum()) > 500
    with pytest.raises(PilosaError):      # the recipe without the Sort child cannot get past the guard
        env.q("i", "Extract(Row(f=1), Rows(field=v))")
    full = oracle(d, "v", d.rows[1], True)[0]
    q = extract_sort_text(sort_text("v", "Row(f=1)", limit=10, desc=True), ("v", "mx", "st"))
    check_table(d, env.q1("i", q), ("v", "mx", "st"), full[:10])
    q = extract_sort_text(sort_text("v", "Row(f=1)", limit=40, offset=100, desc=True), ("v",), offset=35)
    check_table(d, env.q1("i", q), ("v",), full[100:140][35:])
    q = extract_sort_text(sort_text("v", "Row(f=1)", limit=40, desc=True), ("v",), offset=3, limit=10)
    check_table(d, env.q1("i", q), ("v",), full[3:13])
    # the guard applies to what is left after both cuts
    for q, n in ((extract_sort_text(sort_text("v", "Row(f=1)", limit=11), ("v",)), 11),
                 (extract_sort_text(sort_text("v", "Row(f=1)", limit=40), ("v",), offset=3, limit=12), 12)):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        assert str(e.value) == f"Extract(): {n} columns exceed the limit of 10; page with limit= and offset="
    # Sort's own guard, through the nested form
    monkeypatch.setenv("PILOSA_SORT_MAX_COLUMNS", "10")
    with pytest.raises(PilosaError) as e:
        env.q("i", extract_sort_text(sort_text("v", "Row(f=1)", limit=8, offset=3), ("v",)))
    assert str(e.value) == "Sort(): 11 columns exceed the limit of 10; page with limit= and offset="


def test_the_const_row_guard_holds_on_the_coordinating_node_too(env, monkeypatch):
    """The second phase is a ConstRow that other nodes parse from its text and
    guard; the coordinating node applies the same guard, so one node and a
    cluster give the same answer."""
    d = env.data
    monkeypatch.setenv("PILOSA_CONSTROW_MAX_COLUMNS", "10")
    full = oracle(d, "v", d.rows[1])[0]
    check_table(d, env.q1("i", extract_sort_text(sort_text("v", "Row(f=1)", limit=10), ("v",))), ("v",), full[:10])
    with pytest.raises(PilosaError) as e:
        env.q("i", extract_sort_text(sort_text("v", "Row(f=1)", limit=11), ("v",)))
    assert str(e.value) == "ConstRow(): 11 columns exceed the limit of 10"


@pytest.mark.parametrize("q,msg", [
    ("Extract(Sort(), Rows(field=v))", "Sort(): field required"),
    ("Extract(Sort(Row(f=1)), Rows(field=v))", "Sort(): field required"),
    ("Extract(Sort(field=f), Rows(field=v))", 'cannot compute Sort() on non-integer field: "f"'),
    ("Extract(Sort(field=nope), Rows(field=v))", "field not found"),
    ("Extract(Sort(Row(f=1), Row(f=2), field=v), Rows(field=v))", "Sort() only accepts a single bitmap input"),
    ("Extract(Sort(field=v, limit=-1), Rows(field=v))", "Sort(): limit must be a non-negative integer"),
    ("Extract(Sort(field=v, offset=1.5), Rows(field=v))", "Sort(): offset must be a non-negative integer"),
    ("Extract(Sort(field=v, sort-desc=1), Rows(field=v))", "Sort(): sort-desc must be a boolean"),
    ("Extract(Sort(field=v, nth=5), Rows(field=v))", 'Sort(): unknown argument "nth"'),
    ("Extract(Sort(field=v))", "Extract(): at least one Rows(field=) required"),
    ("Extract(Sort(field=v), Row(f=2), Rows(field=v))", "Extract() only accepts a single bitmap input"),
    ("Extract(Sort(field=v), Sort(field=w), Rows(field=v))", "Extract() only accepts a single bitmap input"),
    ("Extract(Sort(field=v), Rows(field=v, limit=3))", "Extract(): Rows() accepts only a field"),
    ("Extract(Sort(field=v), Rows(field=nope))", "field not found"),
    ("Extract(Sort(field=v), Rows(field=v), Rows(v))", 'Extract(): duplicate field "v"'),
    ("Extract(Sort(field=v), Rows(field=v), limit=-1)", "Extract(): limit must be a non-negative integer"),
    ("Extract(Sort(field=v), Rows(field=v), offset=true)", "Extract(): offset must be a non-negative integer"),
    ("Extract(Sort(field=v), Rows(field=v), k=3)", 'Extract(): unknown argument "k"'),
    # the Sort child is checked first
    ("Extract(Sort(field=v, nth=5), Rows(field=v), k=3)", 'Sort(): unknown argument "nth"'),
    # an error of Sort's filter
    ("Extract(Sort(Shift(n=2), field=v), Rows(field=v))", "Shift() requires an input row"),
])
def test_errors_through_the_nested_form(env, q, msg):
    with pytest.raises(PilosaError) as e:
        env.q("i", q)
    assert str(e.value).endswith(msg) and (str(e.value) == msg or "Shift" in q)


def test_nested_use_keeps_the_unknown_call_errors(env):
    for q, name in (("Count(Extract(Sort(field=v, limit=3), Rows(field=v)))", "Extract"),
                    ("Count(Sort(field=v))", "Sort"),
                    ("Count(Intersect(Row(f=1), Sort(field=v)))", "Sort"),
                    ("Sum(Sort(field=v, limit=3), field=v)", "Sort")):
        with pytest.raises(PilosaError) as e:
            env.q("i", q)
        assert str(e.value).endswith(f"unknown call: {name}"), q


def test_a_forwarded_request_is_refused(env):
    q = extract_sort_text(sort_text("v", "Row(f=1)", limit=3), ("v",))
    with pytest.raises(PilosaError) as e:
        env.executor.execute("i", q, shards=[1], opt=ExecOptions(remote=True))
    assert "coordinating node" in str(e.value)


# ---------------------------------------------------------------- encodings keep the order
def test_json_protobuf_and_partial_round_trips_keep_the_order(env):
    from pilosa_amd import wire
    from pilosa_amd.parallel.collectives import TAG_EXTRACT, decode_partial, encode_partial
    from pilosa_amd.server import encoding
    d = env.data
    oc = oracle(d, "v", d.rows[1], True)[0][:25]
    assert (np.diff(oc.astype(np.int64)) < 0).any()
    got = env.q1("i", extract_sort_text(sort_text("v", "Row(f=1)", limit=25, desc=True), ("v", "st", "mx", "bl")))
    js = json.loads(encoding.result_json_bytes(got))
    assert [c["column"] for c in js["columns"]] == oc.tolist()
    assert [c["rows"] for c in js["columns"]] == [list(r) for r in zip(*(cells(d, f, oc) for f in ("v", "st", "mx", "bl")))]
    m = encoding.result_to_pb(got, "Extract")
    assert m.Type == 11 == wire.QUERY_RESULT_TYPE_EXTRACTEDTABLE
    back = encoding.result_from_pb(wire.pb.QueryResult.FromString(m.SerializeToString()))
    assert isinstance(back, ExtractedTable) and back == got and back.columns.tolist() == oc.tolist()
    w = encode_partial(got)
    assert int(w[0]) == TAG_EXTRACT
    back = decode_partial(w)
    assert back == got and back.columns.tolist() == oc.tolist()


def test_keyed_index_and_column_attrs():
    e = Env()
    try:
        e.create_index("k", keys=True)
        e.field("k", "f", keys=True)
        e.field("k", "v", type="int", min=-100, max=100)
        e.field("k", "m", type="mutex", keys=True)
        vals = {"a": 7, "b": -7, "c": 0, "d": 7, "e": 50}
        e.q("k", " ".join(f'Set("{c}", v={x})' for c, x in vals.items()) +
            ' Set("a", f="x") Set("b", f="x") Set("e", f="y") Set("d", f="x") Set("d", f="y") Set("b", m="one")')
        got = e.q1("k", 'Extract(Sort(Row(f="x"), field=v, sort-desc=true), Rows(field=v), Rows(field=f), Rows(field=m))')
        assert got.keys == ["a", "d", "b"] and got.cells(0) == [7, 7, -7]
        assert got.cells(1) == [["x"], ["x", "y"], ["x"]] and got.cells(2) == [None, None, "one"]
        assert got.fields == [("v", "int64"), ("f", "[]string"), ("m", "string")]
        js = e.q1("k", 'Extract(Sort(field=v, limit=4), Rows(field=v), offset=1, limit=2)').to_json()
        assert js["columns"] == [{"column": "c", "rows": [0]}, {"column": "a", "rows": [7]}]
        e.q("k", " ".join(f'SetColumnAttrs("{c}", tag="t{c}")' for c in vals))
        resp = e.executor.execute("k", 'Options(Extract(Sort(Row(f="x"), field=v), Rows(field=v)), columnAttrs=true)')
        assert not resp.column_attr_sets and resp.results[0].keys == ["b", "a", "d"]
    finally:
        e.close()


# ---------------------------------------------------------------- cluster
PAGES = [(None, None, None, None), (None, 60, 10, 30), (20, 70, 5, None), (0, 125, 100, 40), (130, 40, 0, 40),
         (0, 10, 0, 0)]


def test_two_node_cluster_pages_match_numpy():
    from tests.test_percentile import _close, _load_small, _servers
    servers = _servers(2)
    try:
        c, cs, vals, in_f = _load_small(servers)
        owners = {s.node.id: sorted(s.holder.field("i", "v").view("bsig_v").fragments) for s in servers}
        assert all(owners.values()) and sorted(sum(owners.values(), [])) == list(SHARDS), owners
        mask = np.isin(cs, in_f)
        value = dict(zip(cs.tolist(), vals.tolist()))
        member = set(in_f.tolist())
        for desc in (False, True):
            col, v = cs[mask].astype(np.uint64), vals[mask]
            order = np.lexsort((col, ~v if desc else v))
            full = col[order].tolist()
            for s_off, s_lim, e_off, e_lim in PAGES:
                q = extract_sort_text(sort_text("v", "Row(f=1)", limit=s_lim, offset=s_off, desc=desc), ("v", "f"),
                                      offset=e_off, limit=e_lim)
                want = cut(cut(full, s_off or 0, s_lim), e_off or 0, e_lim)
                for s in servers:
                    got = c.query(s.uri, "i", q)["results"][0]
                    assert got["fields"] == [{"name": "v", "type": "int64"}, {"name": "f", "type": "[]uint64"}]
                    assert [x["column"] for x in got["columns"]] == want, (q, s.node.id)
                    assert [x["rows"] for x in got["columns"]] == \
                        [[value[x], [1] if x in member else []] for x in want], q
        page = cut(cut(full, 0, 60), 10, 30)
        assert len({x // SW for x in page}) > 1, "the page holds one node's columns only"
    finally:
        _close(servers)


# ---------------------------------------------------------------- mesh
MESH_QUERIES = ["Extract(Sort(field=v), Rows(field=v), Rows(field=f))",
                "Extract(Sort(field=v, limit=50, offset=80), Rows(field=v), Rows(field=g), limit=30, offset=10)",
                "Extract(Sort(Row(f=1), field=v, sort-desc=true), Rows(field=f), Rows(field=v), limit=20)",
                "Extract(Sort(Not(Row(g=3)), field=v, limit=40, offset=30, sort-desc=true), Rows(field=v), offset=35)",
                "Extract(Sort(Row(g=9), field=v), Rows(field=v))"]


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


def test_two_rank_mesh_pages_equal_host_and_numpy(tmp_path):
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
    col = np.array(sorted(last), np.uint64)
    v = np.array([last[int(c)] for c in col], np.int64)
    order = np.lexsort((col, v))
    full = json.loads(want[0])[0]["columns"]
    assert [x["column"] for x in full] == col[order].tolist() and len(col) > 400
    assert [x["rows"][0] for x in full] == v[order].tolist()
    page = json.loads(want[1])[0]["columns"]
    assert [x["column"] for x in page] == col[order][80:130][10:40].tolist()
    assert len({x["column"] // SW for x in page}) > 1, "the page lies inside one shard"
    assert json.loads(want[4])[0]["columns"] == []
