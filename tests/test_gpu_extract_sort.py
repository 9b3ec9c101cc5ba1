"""Extract(Sort(...), Rows(field=)...) with every phase on the device -- the
bsi_kth descent and K29 for the Sort, K30 for the ConstRow of its columns, the
count pass and K27 / K28 for the fields -- against numpy and against the host
path, on tests/test_gpu_sort.py's fixture: three shards with a gap, depths 11,
21, 32 and 40, and a tie group whose members sit on both sides of the pinned
2047 / 2048 and 8191 / 8192 boundaries, so that either window can end there.
Every answer is exact."""
import numpy as np
import pytest

from pilosa_amd.executor import ExtractedTable

from tests.const_row_util import cut, extract_sort_text
from tests.distinct_util import load
from tests.extract_util import int_cells
from tests.helpers import SW, Env
from tests.sort_util import call_text as sort_text, oracle, tie_group
from tests.test_gpu_extract import set_cells
from tests.test_gpu_sort import FAR, SHARDS, TIE, Data
from tests.test_mesh import _canon

pytestmark = pytest.mark.gpu
COUNTERS = ("sortDevice", "constRowDevice", "extractDevice", "extractRowsDevice")
MX_ROWS = (0, 2, 3, 77, (1 << 40) + 8)


@pytest.fixture(scope="module")
def envs():
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env()
    env.data = d = Data()
    load(env, d)
    env.field("i", "mx", type="mutex")
    rng = np.random.default_rng(6)
    d.mx_has = rng.random(len(d.cols)) < 0.6
    d.mx_row = np.asarray(MX_ROWS, np.uint64)[rng.integers(0, len(MX_ROWS), len(d.cols))]
    env.holder.index("i").field("mx").import_bits(d.mx_row[d.mx_has], d.cols[d.mx_has])
    gpu = GpuExecutor(env.holder, "cuda:0", executor=env.executor)
    env.executor.gpu = gpu
    env.executor.strict_gpu = True        # a device error is an error, not a silent host answer
    yield env, gpu
    env.close()


def mx_cells(d, columns):
    order = np.argsort(d.cols)
    at = order[np.searchsorted(d.cols[order], columns)]
    assert (d.cols[at] == columns).all()
    return [int(r) if ok else None for r, ok in zip(d.mx_row[at].tolist(), d.mx_has[at].tolist())]


def check_table(d, got, fields, columns):
    assert isinstance(got, ExtractedTable) and got.keys is None
    assert got.columns.dtype == np.uint64 and got.columns.tolist() == columns.tolist()
    assert [n for n, _ in got.fields] == list(fields)
    for i, f in enumerate(fields):
        want = set_cells(d, columns) if f == "f" else mx_cells(d, columns) if f == "mx" else int_cells(d, f, columns)
        assert got.cells(i) == want, f


def _host(env, gpu, monkeypatch, q):
    """The same request with every device route declining: the host path."""
    def decline(*a, **k):
        raise NotImplementedError
    with monkeypatch.context() as m:
        for name in ("plan", "bsi_sort", "bsi_extract"):
            m.setattr(gpu, name, decline)
        s0 = gpu.stats()
        r = env.q1("i", q)
        assert all(gpu.stats()[k] == s0[k] for k in COUNTERS)
    return r


def _device(env, gpu, q, moved=COUNTERS):
    """The request, with each of the ``moved`` counters moving and no other."""
    s0 = gpu.stats()
    r = env.q1("i", q)
    s1 = gpu.stats()
    for k in COUNTERS:
        assert (s1[k] > s0[k]) == (k in moved), f"{k}: {s0[k]} -> {s1[k]}: {q[:80]}"
    return r


FIELDS = ("v", "m", "d32", "f", "mx")


@pytest.mark.parametrize("field", ["v", "m", "d32"])
@pytest.mark.parametrize("desc", [False, True])
def test_device_equals_numpy_and_host(envs, monkeypatch, field, desc):
    env, gpu = envs
    d = env.data
    for filt, mask in (("Row(f=1)", d.rows[1]), ("", np.ones(len(d.cols), bool)), ("Not(Row(f=4))", ~d.rows[4])):
        full, vals = oracle(d, field, mask, desc)
        # 80 columns around the first change of value past position 40: the order is not the column order
        off = int(np.flatnonzero(np.diff(vals[40:]))[0]) + 1
        q = extract_sort_text(sort_text(field, filt, limit=80, offset=off, desc=desc if desc else None), FIELDS)
        got = _device(env, gpu, q)
        check_table(d, got, FIELDS, full[off:off + 80])
        assert (np.diff(full[off:off + 80].astype(np.int64)) < 0).any(), "the sorted order is the column order"
        assert _canon([got]) == _canon([_host(env, gpu, monkeypatch, q)]), q
    # int fields alone: no set-like pass
    q = extract_sort_text(sort_text(field, "Row(f=1)", limit=30, desc=desc), ("v", "d32"))
    check_table(d, _device(env, gpu, q, moved=COUNTERS[:3]), ("v", "d32"), oracle(d, field, d.rows[1], desc)[0][:30])
    # set-like fields alone: no int pass
    q = extract_sort_text(sort_text(field, "Row(f=1)", limit=30, desc=desc), ("mx", "f"))
    check_table(d, _device(env, gpu, q, moved=("sortDevice", "constRowDevice", "extractRowsDevice")), ("mx", "f"),
                oracle(d, field, d.rows[1], desc)[0][:30])


@pytest.mark.parametrize("field", ["v", "d32"])
@pytest.mark.parametrize("desc", [False, True])
def test_cuts_before_inside_and_after_the_tie_group(envs, monkeypatch, field, desc):
    env, gpu = envs
    d = env.data
    full, vals = oracle(d, field, d.rows[1], desc)
    lo, hi = tie_group(vals, TIE[field])
    group = full[lo:hi].tolist()
    # Sort's window ends right after the members 2047, 2048, 8191, 8192, the first far column,
    # before the group, at its last member and after it; the table holds the 25 columns before the cut
    ends = [lo + group.index(c) + 1 for c in (2047, 2048, 8191, 8192, FAR[0])] + [lo, hi, hi + 3]
    assert all(e > 25 for e in ends)
    for k, end in enumerate(ends):
        q = extract_sort_text(sort_text(field, "Row(f=1)", limit=25, offset=end - 25, desc=desc), (field, "mx"))
        got = _device(env, gpu, q)
        check_table(d, got, (field, "mx"), full[end - 25:end])
        if k % 3 == 0:
            assert _canon([got]) == _canon([_host(env, gpu, monkeypatch, q)]), q
    # Extract's own window ends at the same members, Sort's beyond them
    for c in (2047, 8191):
        end = lo + group.index(c) + 1
        q = extract_sort_text(sort_text(field, "Row(f=1)", limit=hi + 10, desc=desc), (field, "f"),
                              offset=end - 10, limit=10)
        check_table(d, _device(env, gpu, q), (field, "f"), full[end - 10:end])
    # Extract's offset mid-answer, with and without its limit
    for s_off, s_lim, e_off, e_lim in ((lo - 5, 60, 20, 15), (3, 100, 60, None), (lo + 2, 40, 39, 5), (0, 50, 49, None)):
        q = extract_sort_text(sort_text(field, "Row(f=1)", limit=s_lim, offset=s_off, desc=desc), (field, "mx", "f"),
                              offset=e_off, limit=e_lim)
        got = _device(env, gpu, q)
        check_table(d, got, (field, "mx", "f"), cut(cut(full, s_off, s_lim), e_off, e_lim))
        assert _canon([got]) == _canon([_host(env, gpu, monkeypatch, q)]), q


def test_empty_answers_launch_no_second_phase(envs):
    env, gpu = envs
    for q in (extract_sort_text(sort_text("v", "Row(f=9)", limit=5), ("v", "f")),
              extract_sort_text(sort_text("v", "Row(f=1)", limit=5), ("v", "f"), offset=5),
              extract_sort_text(sort_text("v", "Row(f=1)", limit=5), ("v", "f"), limit=0)):
        got = _device(env, gpu, q, moved=("sortDevice",))
        assert got == ExtractedTable([("v", "int64"), ("f", "[]uint64")])


def test_a_depth_40_sort_field_keeps_the_rest_on_the_device(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    for desc in (False, True):
        q = extract_sort_text(sort_text("big", "Row(f=1)", limit=40, desc=desc), ("big", "v", "mx"))
        # big itself is gathered on the host over the device's columns; v and mx stay on the device
        got = _device(env, gpu, q, moved=COUNTERS[1:])
        check_table(d, got, ("big", "v", "mx"), oracle(d, "big", d.rows[1], desc)[0][:40])
        assert _canon([got]) == _canon([_host(env, gpu, monkeypatch, q)])


def test_the_extract_guard_sees_the_sorted_window_not_the_filter(envs, monkeypatch):
    env, gpu = envs
    d = env.data
    monkeypatch.setenv("PILOSA_EXTRACT_MAX_COLUMNS", "10")
    assert int(d.rows[1].sum()) > 10000
    q = extract_sort_text(sort_text("v", "Row(f=1)", limit=10, desc=True), ("v", "f", "mx"))
    check_table(d, _device(env, gpu, q), ("v", "f", "mx"), oracle(d, "v", d.rows[1], True)[0][:10])


def test_after_writes():
    """After device writes: a value that enters the top k brings its other fields along."""
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env(gpu=lambda h: GpuExecutor(h, "cuda:0"))
    try:
        gpu = env.executor.gpu
        gpu.executor = env.executor
        env.executor.strict_gpu = True
        env.create_index("i")
        env.field("i", "f")
        env.field("i", "v", type="int", min=-100000, max=100000)
        env.field("i", "w", type="int", min=0, max=1000)
        env.field("i", "mx", type="mutex")
        rng = np.random.default_rng(3)
        cols = np.sort(np.concatenate([s * SW + rng.choice(SW // 2, 3000, replace=False) for s in SHARDS]))
        vals = rng.integers(-900, 901, len(cols))
        ws = rng.integers(0, 1001, len(cols))
        idx = env.holder.index("i")
        idx.field("v").import_values(cols.astype(np.uint64), vals)
        idx.field("w").import_values(cols.astype(np.uint64), ws)
        idx.field("f").import_bits(np.ones(len(cols), np.uint64), cols.astype(np.uint64))
        idx.field("mx").import_bits((cols % 7).astype(np.uint64), cols.astype(np.uint64))
        cur = {c: [v, w, c % 7] for c, v, w in zip(cols.tolist(), vals.tolist(), ws.tolist())}
        q = {desc: extract_sort_text(sort_text("v", "Row(f=1)", limit=10, desc=desc), ("v", "w", "mx"))
             for desc in (False, True)}

        def check_top():
            for desc in (False, True):
                got = _device(env, gpu, q[desc], moved=COUNTERS)
                order = sorted(cur, key=lambda c: (-cur[c][0] if desc else cur[c][0], c))[:10]
                assert got.columns.tolist() == order
                assert [list(r) for r in zip(got.cells(0), got.cells(1), got.cells(2))] == [cur[c] for c in order]
            return set(env.q1("i", q[False]).columns.tolist())
        top = check_top()
        enters = next(int(c) for c in cols[::-1] if int(c) not in top)
        env.q("i", f"Set({enters}, v=-77777) Set({enters}, w=999) Set({enters}, mx=5)")
        cur[enters] = [-77777, 999, 5]
        top = check_top()
        assert enters in top
        leaves = next(c for c in sorted(top) if c != enters)
        env.q("i", f"Set({leaves}, v=88888)")
        cur[leaves][0] = 88888
        assert leaves not in check_top()
    finally:
        env.close()
