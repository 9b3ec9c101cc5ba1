"""GroupBy(..., aggregate=Sum(field=)) on the host path: every group carries
the sum of an int field over its columns.  Pilosa v1.3 has no such argument,
so every answer is pinned to a numpy computation over the generated columns
(exact integers), and the encodings of a GroupBy without the argument are
pinned to the bytes they had before it existed."""
import json

import numpy as np
import pytest

from pilosa_amd.errors import PilosaError
from pilosa_amd.executor import FieldRow, GroupCount, QueryResponse, merge_group_counts

from tests.groupby_sum_util import SHARDS, Data, call_text, flat
from tests.helpers import SW, Env

FILTERS = ["", "Row(f=1)", "Intersect(Row(f=1), Row(g=1))"]
FIELDS = {1: ["a"], 2: ["a", "b"], 3: ["a", "b", "c"]}


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.data = Data(n=1500)
    e.data.load(e)
    yield e
    e.close()


def test_fixture(env):
    d = env.data
    assert sorted(set((d.cols // np.uint64(SW)).tolist())) == list(SHARDS)
    assert (d.vals["v"][d.has["v"]] < 0).any() and not d.has["w"][::5].any()
    assert env.holder.field("i", "w").bsi_group("w").base == 100
    novalue = [g for g in d.expected(["a"], "w") if g[1] > 0 and g[3] == 0]
    assert novalue == [((4,), novalue[0][1], 0, 0)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_host_path_matches_numpy(env, k, filt):
    for vf in ("v", "w", "big"):
        want = env.data.expected(FIELDS[k], vf, filt)
        assert len(want) >= (8 if k == 1 else 30)
        got = env.q1("i", call_text(FIELDS[k], vf, filt))
        assert all(isinstance(g, GroupCount) for g in got)
        assert flat(got) == want, (k, vf, filt)


@pytest.mark.parametrize("kw", [{"limit": 7}, {"previous": [2, 3]}, {"previous": [4, 1], "limit": 5},
                                {"limit": 11, "offset": 3}, {"offset": 40}])
def test_paging(env, kw):
    for filt in ("", "Row(f=1)"):
        want = env.data.expected(["a", "b"], "w", filt, **kw)
        assert want
        assert flat(env.q1("i", call_text(["a", "b"], "w", filt, **kw))) == want


def test_child_rows_arguments(env):
    d = env.data
    got = env.q1("i", call_text(None, "v", children=["Rows(a, limit=3)", "Rows(b)"]))
    assert flat(got) == d.expected(["a", "b"], "v", keep={"a": [1, 2, 3]})
    col = int(d.cols[d.rows["a"][2] & d.rows["b"][1]][0])
    in_a = [r for r, m in d.rows["a"].items() if col in d.cols[m]]
    assert 2 in in_a
    got = env.q1("i", call_text(None, "w", "Row(f=1)", children=[f"Rows(a, column={col})", f"Rows(b, column={col})"]))
    assert flat(got) == d.expected(["a", "b"], "w", "Row(f=1)", keep={"a": in_a, "b": [1]})


def test_same_groups_without_aggregate(env):
    for k in (1, 2, 3):
        for kw in ({}, {"limit": 4}, {"previous": [2, 1, 1][:k]}):
            plain = env.q1("i", call_text(FIELDS[k], None, "Row(f=1)", **kw))
            agg = env.q1("i", call_text(FIELDS[k], "v", "Row(f=1)", **kw))
            assert all(g.sum is None and g.sum_count is None for g in plain)
            assert [(g.group, g.count) for g in plain] == [(g.group, g.count) for g in agg] and plain
            assert flat(plain) == env.data.expected(FIELDS[k], None, "Row(f=1)", **kw)


def test_missing_bsi_fragment_contributes_nothing(env):
    """An int field without a fragment in a shard: the groups of that shard
    still appear, with 0 / 0 from it."""
    env.field("i", "sparse", type="int", min=0, max=100)
    d = env.data
    cols = d.cols[d.rows["a"][2] & (d.cols < np.uint64(SW))][:10]     # shard 0 only
    env.holder.index("i").field("sparse").import_values(cols, np.arange(10, 20))
    got = flat(env.q1("i", "GroupBy(Rows(a), aggregate=Sum(field=sparse))"))
    val = dict(zip(cols.tolist(), range(10, 20)))
    want = []
    for key, n, _, _ in d.expected(["a"], "v"):
        have = [val[c] for c in d.cols[d.rows["a"][key[0]]].tolist() if c in val]
        want.append((key, n, sum(have), len(have)))
    assert want[1][2:] == (sum(range(10, 20)), 10)
    only3 = flat(env.q1("i", "Options(GroupBy(Rows(a), aggregate=Sum(field=sparse)), shards=[3])"))
    assert got == want and only3 and all(g[2:] == (0, 0) for g in only3)


# ---------------------------------------------------------------- encodings
PLAIN = [GroupCount([FieldRow("a", 1), FieldRow("b", 0)], 12), GroupCount([FieldRow("a", 2), FieldRow("b", 4, "k")], 3)]
# what the code wrote for PLAIN before the aggregate existed
PLAIN_JSON = (b'{"results":[[{"group":[{"field":"a","rowID":1},{"field":"b","rowID":0}],"count":12},'
              b'{"group":[{"field":"a","rowID":2},{"field":"b","rowKey":"k"}],"count":3}]]}\n')
PLAIN_PB = bytes.fromhex("3007420e0a050a016110010a030a0162100c42130a050a016110020a080a016210041a016b1003")
PLAIN_PARTIAL = bytes.fromhex("0600000000000000010000000000000002000000000000000500000000000000"
                              "92a161a16200000001000000000000000000000000000000" "0c00000000000000")
PLAIN_MSGPACK = bytes.fromhex("c713049292c7050693a16101a0c7050693a16200a00c")
WITH = [GroupCount([FieldRow("a", 1), FieldRow("b", 0)], 12, -77, 9), GroupCount([FieldRow("a", 2), FieldRow("b", 4)], 3, 0, 0)]


def test_bytes_without_aggregate_are_unchanged():
    from pilosa_amd.parallel import collectives as C
    from pilosa_amd.server import encoding
    assert encoding.response_json_bytes(QueryResponse([PLAIN])) == PLAIN_JSON
    assert encoding.result_to_pb(PLAIN, "GroupBy").SerializeToString() == PLAIN_PB
    assert C.encode_partial(PLAIN[:1]).tobytes() == PLAIN_PARTIAL and C.TAG_GROUPS == 6
    assert C.encode(PLAIN[0]) == PLAIN_MSGPACK
    assert repr(PLAIN[0]) == "GroupCount([FieldRow('a', 1), FieldRow('b', 0)], 12)"


def test_json_and_protobuf_round_trip():
    from pilosa_amd.server import encoding
    from pilosa_amd.wire import pb
    body = encoding.response_json_bytes(QueryResponse([WITH]))
    assert body == (b'{"results":[[{"group":[{"field":"a","rowID":1},{"field":"b","rowID":0}],"count":12,"sum":-77,'
                    b'"sumCount":9},{"group":[{"field":"a","rowID":2},{"field":"b","rowID":4}],"count":3,"sum":0,'
                    b'"sumCount":0}]]}\n')
    assert json.loads(body)["results"][0][1] == {"group": [{"field": "a", "rowID": 2}, {"field": "b", "rowID": 4}],
                                                 "count": 3, "sum": 0, "sumCount": 0}
    wire = encoding.result_to_pb(WITH, "GroupBy").SerializeToString()
    m = pb.QueryResult()
    m.ParseFromString(wire)
    assert [(g.Sum, g.SumCount, g.HasSum) for g in m.GroupCounts] == [(-77, 9, True), (0, 0, True)]
    back = encoding.result_from_pb(m)
    assert back == WITH and (back[1].sum, back[1].sum_count) == (0, 0)     # sum 0 is not "no aggregate"
    plain = encoding.result_from_pb(encoding.result_to_pb(PLAIN, "GroupBy"))
    assert plain == PLAIN and plain[0].sum is None and plain[0].sum_count is None
    assert WITH[0] != PLAIN[0] and GroupCount(PLAIN[0].group, 12, -77, 9) == WITH[0]
    assert GroupCount(PLAIN[0].group, 12, -77, 8) != WITH[0]
    assert repr(WITH[0]) == "GroupCount([FieldRow('a', 1), FieldRow('b', 0)], 12, sum=-77, sum_count=9)"


def test_partial_round_trip_with_sums():
    from pilosa_amd.parallel import collectives as C
    groups = WITH + [GroupCount([FieldRow("a", 1 << 63), FieldRow("b", 7)], 1 << 40, -(1 << 62), 1 << 40)]
    w = C.encode_partial(groups)
    assert int(w[0]) == C.TAG_GROUPS_SUM != C.TAG_GROUPS and list(w[1:3]) == [3, 2]
    assert len(w) == 4 + (int(w[3]) + 7) // 8 + 3 * (2 + 3)                 # k + 3 int64 columns per group
    assert C.decode_partial(w) == groups
    assert C.decode_partial(C.encode_partial(PLAIN[:1])) == PLAIN[:1]
    keyed = [GroupCount([FieldRow("a", 2, "k")], 3, 5, 1)]                  # a key: the msgpack codec
    assert int(C.encode_partial(keyed)[0]) == C.TAG_MSGPACK and C.decode_partial(C.encode_partial(keyed)) == keyed
    assert C.decode(C.encode(WITH)) == WITH


def _g(key, n, s=None, c=None):
    return GroupCount([FieldRow("a", key)], n, s, c)


def test_merge_group_counts_adds_sums():
    a = [_g(1, 2, 10, 2), _g(3, 1, -4, 1), _g(5, 7, 0, 0)]
    b = [_g(1, 3, -25, 3), _g(2, 1, 6, 1), _g(5, 1, 9, 1), _g(8, 2, 1, 2)]
    want = [_g(1, 5, -15, 5), _g(2, 1, 6, 1), _g(3, 1, -4, 1), _g(5, 8, 9, 1), _g(8, 2, 1, 2)]
    assert merge_group_counts(a, b, 1 << 62) == want
    assert merge_group_counts(a, b, 4) == want[:4] and merge_group_counts(b, a, 1) == want[:1]
    big = merge_group_counts([_g(1, 1, (1 << 63) - 1, 1)], [_g(1, 1, 1, 1)], 10)
    assert flat(big) == [((1,), 2, -(1 << 63), 2)]                          # int64 wrap, as Sum
    plain = merge_group_counts([_g(1, 2)], [_g(1, 3)], 10)
    assert plain == [_g(1, 5)] and plain[0].sum is None


# ---------------------------------------------------------------- errors, parsers
@pytest.mark.parametrize("q,msg", [
    ("GroupBy(Rows(a), aggregate=3)", "GroupBy(): aggregate must be a call, but got int"),
    ("GroupBy(Rows(a), aggregate=\"Sum\")", "GroupBy(): aggregate must be a call, but got str"),
    ("GroupBy(Rows(a), aggregate=Min(field=v))", "GroupBy(): aggregate must be Sum(), but got Min()"),
    ("GroupBy(Rows(a), aggregate=Sum())", "Sum(): field required"),
    ("GroupBy(Rows(a), aggregate=Sum(field=nope))", "Sum(): field not found: nope"),
    ("GroupBy(Rows(a), aggregate=Sum(field=f))", "Sum(): field f is not an int field"),
    ("GroupBy(Rows(a), aggregate=Sum(Row(f=1), field=v))",
     "Sum() inside aggregate= accepts no bitmap input, use GroupBy's filter="),
])
def test_errors(env, q, msg):
    with pytest.raises(PilosaError) as e:
        env.q("i", q)
    assert str(e.value) == msg


def test_parsers_agree_and_canonical_text():
    from pilosa_amd import _pql
    from pilosa_amd.pql import Call
    from pilosa_amd.pql import parser as P
    assert P._native is _pql, "parse_string does not use the native parser"
    text = "GroupBy(Rows(a), Rows(field=b), filter=Row(f=1), limit=3, aggregate=Sum(field=v))"
    a, b = _pql.parse_calls(text), P.parse_string_py(text).calls
    want = Call("GroupBy", {"filter": Call("Row", {"f": 1}), "limit": 3, "aggregate": Call("Sum", {"field": "v"})},
                [Call("Rows", {"_field": "a"}), Call("Rows", {"field": "b"})])
    assert list(a) == b == [want] == P.parse_string(text).calls
    canon = 'GroupBy(Rows(_field="a"), Rows(field="b"), aggregate=Sum(field="v"), filter=Row(f=1), limit=3)'
    assert str(a[0]) == str(b[0]) == canon
    assert P.parse_string(canon).calls == P.parse_string_py(canon).calls == [want]   # what a remote node receives


# ---------------------------------------------------------------- cluster
def test_two_node_cluster_matches_numpy():
    from tests.test_percentile import _close, _servers
    from pilosa_amd.server.client import InternalClient
    servers = _servers(2)
    try:
        c, s0 = InternalClient(), servers[0]
        c.create_index(s0.uri, "i")
        c.create_field(s0.uri, "i", "a", {"type": "set"})
        c.create_field(s0.uri, "i", "f", {"type": "set"})
        c.create_field(s0.uri, "i", "v", {"type": "int", "min": -1000, "max": 1000})
        import time
        deadline = time.time() + 5
        while time.time() < deadline and not all(s.holder.field("i", "v") is not None for s in servers):
            time.sleep(0.05)
        rng = np.random.default_rng(9)
        cols = np.concatenate([s * SW + rng.choice(5000, 100, replace=False) for s in SHARDS])
        vals = rng.integers(-1000, 1001, len(cols))
        has = np.arange(len(cols)) % 4 != 0
        arow = rng.integers(1, 5, len(cols))
        in_f = rng.random(len(cols)) < 0.5
        q = " ".join([f"Set({int(col)}, v={int(v)})" for col, v in zip(cols[has], vals[has])] +
                     [f"Set({int(col)}, a={int(r)})" for col, r in zip(cols, arow)] +
                     [f"Set({int(col)}, f=1)" for col in cols[in_f]])
        assert all(c.query(s0.uri, "i", q)["results"])
        owners = {s.node.id: sorted(s.holder.field("i", "v").view("bsig_v").fragments) for s in servers}
        assert all(owners.values()) and sorted(sum(owners.values(), [])) == list(SHARDS), owners
        for filt, m in (("", np.ones(len(cols), bool)), ("Row(f=1)", in_f)):
            want = [{"group": [{"field": "a", "rowID": r}], "count": int((m & (arow == r)).sum()),
                     "sum": int(vals[m & has & (arow == r)].sum()), "sumCount": int((m & has & (arow == r)).sum())}
                    for r in range(1, 5)]
            text = call_text(["a"], "v", filt)
            for s in servers:
                assert c.query(s.uri, "i", text)["results"][0] == want, (text, s.node.id)
            assert c.query(s0.uri, "i", call_text(["a"], "v", filt, limit=2))["results"][0] == want[:2]
            # the protobuf bodies between nodes: each node's own shards, merged as map/reduce does
            parts = [c.query_node(s.node, "i", text, owners[s.node.id])[0] for s in servers]
            assert all(g.sum is not None for p in parts for g in p)
            got = merge_group_counts(parts[0], parts[1], 1 << 62)
            assert flat(got) == [((g["group"][0]["rowID"],), g["count"], g["sum"], g["sumCount"]) for g in want]
    finally:
        _close(servers)
