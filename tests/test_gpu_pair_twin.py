"""Pair kernel (pair_kernels.hip), 64 queries per wave: bitmap twins of dense
array rows (TWN), and the LDS bitmap's clear between stagings.  Every count
is compared exactly with the host roaring oracle, and the flagged kernels'
partial buffers with the plain v6 kernel's."""
import numpy as np
import pytest

from pilosa_amd import _roaring as R

pytestmark = pytest.mark.gpu

EDGE = np.array([0, 31, 32, 65535], np.int64)
PARTNER_N = (1, 8, 9, 64, 65, 511, 512, 513)
PARTNERS = list(range(10, 10 + len(PARTNER_N)))   # rows 10..17, row 18: ~3000 values
D0, D1, D2, BM, RUNROW, P3000 = 0, 1, 2, 3, 4, 18


def _vals(rng, n):
    """n distinct 16-bit values, the edge values 0, 31, 32, 65535 first."""
    if n == "run":
        return np.concatenate([np.arange(0, 40000), [65535]])
    if n <= 4:
        return EDGE[:n].copy()
    return np.sort(np.concatenate([EDGE, rng.choice(np.arange(33, 65535), n - 4, replace=False)]))


def _spec(T, nkeys):
    """row -> per shard -> per key container size.  D0 / D1 / D2 qualify for
    a twin (mostly arrays, mean above T); D2 holds one container below T."""
    if nkeys == 1:   # one key per shard: the sizes spread over the two shards
        spec = {D0: [[T], [T + 1]], D1: [[4095], [4096]], D2: [[4096], [T - 1]], BM: [[4097], [30000]],
                RUNROW: [["run"], [4000]], P3000: [[3000], [50]]}
    else:
        dense = [T, T + 1, 4095, 4096, 4097, "run"]
        spec = {D0: [dense, dense], D1: [dense, dense], D2: [[4000] * 6, [T - 1] + [4000] * 5],
                BM: [[4097] + [30000] * 5] * 2, RUNROW: [["run", 4000] * 3] * 2,
                P3000: [[3000, 3000, 50, 50, 50, 50]] * 2}
    for row, n in zip(PARTNERS, PARTNER_N):
        spec[row] = [[n] * nkeys, [n] * nkeys]
    return spec


def _build(rng, T, nkeys, cpr):
    """(frags, cont) for two shards; cont[(shard, row, key)] = its values."""
    cont = {}
    frags = []
    for s in range(2):
        pos, runs = [], []
        for row, per_shard in _spec(T, nkeys).items():
            for j, n in enumerate(per_shard[s]):
                v = _vals(rng, n)
                cont[(s, row, j)] = v
                (runs if n == "run" else pos).append(
                    (np.uint64(row) * np.uint64(cpr) + np.uint64(j)) * np.uint64(65536) + v.astype(np.uint64))
        # only the run containers are optimised: a 4096-value container stays an array
        b = R.Bitmap(np.concatenate(pos))
        if runs:
            rb = R.Bitmap(np.concatenate(runs))
            rb.optimize()
            b = b.union(rb)
        frags.append(b)
    return frags, cont


def _pairs(rng):
    """70 (a, b) row pairs: runs of a twinned A, both sides twinned, a bitmap
    A with twinned B's, an untwinned array A with twinned B's, one-offs."""
    prs = [(D0, p) for p in PARTNERS + [P3000]]
    prs += [(D0, D1), (D0, D2), (D0, BM), (D0, RUNROW)]
    prs += [(BM, D1), (BM, D2), (BM, P3000), (BM, 10), (BM, 12), (BM, 15), (BM, RUNROW)]
    prs += [(17, D1), (17, D2), (17, 11), (17, 13), (17, 16), (17, BM), (17, P3000)]
    prs += [(D1, 14), (D2, 16), (RUNROW, D2), (D1, D1), (P3000, D1)]
    rows = [RUNROW, P3000] + PARTNERS   # the fill leaves the dense rows' frequencies (their A / B side) alone
    while len(prs) < 70:
        prs.append((int(rng.choice(rows)), int(rng.choice(rows))))
    return prs


def _want(frags, prs, width):
    rows = {}

    def row(s, r):
        if (s, r) not in rows:
            rows[(s, r)] = frags[s].offset_range(0, r * width, (r + 1) * width)
        return rows[(s, r)]
    return np.array([sum(row(s, a).intersection_count(row(s, b)) for s in range(len(frags))) for a, b in prs])


def _partials(eng, handle, variant):
    """The pair kernel's partial buffer for the batch's AND2 part."""
    import torch
    Q, S, tv, parts = handle[:4]
    (tp, ti, kind, n), = parts
    pairs = torch.empty(S * 16 * n * 2, dtype=torch.int32, device=eng.device)
    partial = torch.full((S * 16 * n,), -7, dtype=torch.int32, device=eng.device)
    eng.ext.and2_count(tp, tv, S, pairs, partial, 64, variant)
    return partial.cpu().numpy()


def _sorted_rows(handle):
    """(A dense row, B dense row) of the batch in kernel order."""
    from pilosa_amd.ops.device import QPROG_DTYPE
    progs = handle[3][0][0].cpu().numpy().view(QPROG_DTYPE)
    return progs["leaf_row"][:, 0].copy(), progs["leaf_row"][:, 1].copy()


def _twin_bits(view):
    gen, buf, slot, _, rows, cutoff = view._twin
    return rows, buf.view(len(rows), view.S, 16, 1024).cpu().numpy()


def _check_twin_content(view, cont, nkeys):
    rows, tw = _twin_bits(view)
    for r, d in enumerate(rows.tolist()):
        rid = int(view.rows[d])
        for s in range(view.S):
            for j in range(16):
                want = np.zeros(65536, bool)
                if (s, rid, j) in cont:
                    want[cont[(s, rid, j)]] = True
                bits = np.unpackbits(tw[r, s, j].view(np.uint8), bitorder="little").astype(bool)
                assert np.array_equal(bits, want), (rid, s, j)


@pytest.mark.parametrize("nkeys,cpr", [(6, 16), (1, 1)], ids=["width20", "width16"])
def test_twin_counts_match_host(nkeys, cpr):
    import torch
    from pilosa_amd.ops.device import DeviceView, GpuEngine, Leaf, Op

    T = DeviceView.TWIN_CUTOFF
    rng = np.random.default_rng(21)
    frags, cont = _build(rng, T, nkeys, cpr)
    kinds = {t for f in frags for _, t, _ in f.container_info()}
    assert kinds == {"array", "bitmap", "run"}
    dev = torch.device("cuda:0")
    view = DeviceView.from_bitmaps(frags, dev, shards=[0, 1], cpr=cpr)
    prs = _pairs(np.random.default_rng(5))
    exprs = [Op("and", (Leaf(view, a), Leaf(view, b))) for a, b in prs]
    want = _want(frags, prs, cpr * 65536)
    eng = GpuEngine(dev)
    eng.and2_cq = 64
    handle = eng.prepare_count(exprs)
    assert view.twin_fresh() and handle[4] == 2
    twinned = set(int(view.rows[d]) for d in view._twin[4].tolist())
    assert twinned == {D0, D1, D2}
    assert int(view.viewdev()["twin"]) != 0 and int(view.viewdev()["twin_cutoff"]) == T
    _check_twin_content(view, cont, nkeys)
    # the batch holds every case: twinned A only / B only / both, a bitmap A
    # with a twinned B, runs of equal A and one-off pairs
    ra, rb = _sorted_rows(handle)
    ta = np.isin(view.rows[ra], list(twinned))
    tb = np.isin(view.rows[rb], list(twinned))
    assert (ta & ~tb).any() and (~ta & tb).any() and (ta & tb).any()
    assert ((view.rows[ra] == BM) & tb).any()
    runs = np.diff(np.flatnonzero(np.concatenate([[True], ra[1:] != ra[:-1], [True]])))
    assert (runs == 1).any() and (runs > 4).any()
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want)
    base = _partials(eng, handle, 6)
    assert (base != -7).all()
    for variant in eng.ext.PAIR_VARIANTS:   # 63 ships
        np.testing.assert_array_equal(_partials(eng, handle, variant), base, err_msg=f"variant {variant}")
    # without twins the flagged kernels take the array paths
    plain = GpuEngine(dev)
    plain.and2_cq = 64
    plain.use_twin = False
    np.testing.assert_array_equal(plain.count(exprs), want)


def test_twin_goes_stale_on_write_and_is_rebuilt():
    import torch
    from pilosa_amd.ops.device import DeviceView, GpuEngine, Leaf, Op

    T = DeviceView.TWIN_CUTOFF
    rng = np.random.default_rng(22)
    frags, cont = _build(rng, T, 6, 16)
    dev = torch.device("cuda:0")
    view = DeviceView.from_bitmaps(frags, dev, shards=[0, 1], patchable=True)
    prs = _pairs(np.random.default_rng(5))
    exprs = [Op("and", (Leaf(view, a), Leaf(view, b))) for a, b in prs]
    eng = GpuEngine(dev)
    eng.and2_cq = 64
    np.testing.assert_array_equal(eng.count(exprs), _want(frags, prs, 1 << 20))
    assert view.twin_fresh()
    # a device write into a twinned row (key 1 of D0, shard 1: T + 1 -> T + 41 values)
    new = np.setdiff1d(np.arange(1000, 1400), cont[(1, D0, 1)])[:40]
    pos = (np.uint64(D0) << np.uint64(20)) + np.uint64(65536) + new.astype(np.uint64)
    assert view.apply_positions(1, pos, clear=False)
    frags[1].add_many(pos, True)
    cont[(1, D0, 1)] = np.union1d(cont[(1, D0, 1)], new)
    want = _want(frags, prs, 1 << 20)
    assert not view.twin_fresh() and int(view.viewdev()["twin"]) == 0 and int(view.viewdev()["twin_slot"]) == 0
    # within TWIN_MIN_INTERVAL_S the stale twin is neither passed nor rebuilt
    handle = eng.prepare_count(exprs)
    assert handle[4] == 0 and not view.twin_fresh()
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want)
    view.TWIN_MIN_INTERVAL_S = 0.0
    handle = eng.prepare_count(exprs)
    assert handle[4] == 2 and view.twin_fresh()
    _check_twin_content(view, cont, 6)
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want)


def test_twin_only_for_the_64_query_wave_kernel():
    import torch
    from pilosa_amd.ops.device import DeviceView, GpuEngine, Leaf, Op

    rng = np.random.default_rng(23)
    frags, _ = _build(rng, DeviceView.TWIN_CUTOFF, 1, 1)
    dev = torch.device("cuda:0")
    view = DeviceView.from_bitmaps(frags, dev, shards=[0, 1], cpr=1)
    prs = _pairs(np.random.default_rng(5))
    exprs = [Op("and", (Leaf(view, a), Leaf(view, b))) for a, b in prs]
    eng = GpuEngine(dev)   # 70 queries: the serving-size kernels, no twin is built
    np.testing.assert_array_equal(eng.count(exprs), _want(frags, prs, 65536))
    assert getattr(view, "_twin", None) is None


# ---------------------------------------------------------------- restaging

def _restage_case(rng):
    """One shard, key 0.  A rows in kernel order (ascending row id): small,
    small, large array, bitmap, small, small, a one-off array & bitmap pair
    (stages B), small, small.  Every B holds all the values the bitmap staged
    BEFORE its A held, so a bit left behind changes the count."""
    a_n = {0: 1, 1: 8, 2: 3000, 3: 4500, 4: 9, 5: 511, 6: 400, 7: 512, 8: 64}
    rowvals = {}
    for k, n in a_n.items():   # disjoint value ranges: stale bits never hide in A's own
        rowvals[k] = np.sort(rng.choice(np.arange(k * 6000, k * 6000 + 6000), n, replace=False))
    rowvals[30] = np.sort(rng.choice(65536, 5000, replace=False))   # the one-off pair's bitmap B
    prs = [(6, 30)]
    prev = np.zeros(0, np.int64)
    for k in sorted(a_n):
        if k == 6:
            prev = rowvals[30]      # what the staged bitmap holds after the one-off pair
            continue
        for t in range(2):
            b = 10 + 2 * k + t
            own = rowvals[k][t::2] if len(rowvals[k]) > 1 else rowvals[k]
            rowvals[b] = np.union1d(prev, own)
            prs.append((k, b))
        prev = rowvals[k]
    pos = np.concatenate([np.uint64(r) * np.uint64(1 << 20) + v.astype(np.uint64) for r, v in rowvals.items()])
    return R.Bitmap(pos), a_n, prs


def test_restaging_leaves_no_stale_bits():
    import torch
    from pilosa_amd.ops.device import DeviceView, GpuEngine, Leaf, Op

    rng = np.random.default_rng(24)
    frag, a_n, prs = _restage_case(rng)
    info = {(k >> 4, k & 15): t for k, t, _ in frag.container_info()}
    assert info[(3, 0)] == "bitmap" and info[(30, 0)] == "bitmap" and info[(2, 0)] == "array"
    dev = torch.device("cuda:0")
    view = DeviceView.from_bitmaps([frag], dev, shards=[0])
    exprs = [Op("and", (Leaf(view, a), Leaf(view, b))) for a, b in prs]
    want = _want([frag], prs, 1 << 20)
    assert (want > 0).all()
    eng = GpuEngine(dev)
    eng.and2_cq = 64
    # the plain kernel walks the A sequence with a clear per staging
    eng.and2_variant = 6
    eng.use_twin = False
    handle = eng.prepare_count(exprs)
    ra, _ = _sorted_rows(handle)
    order = [int(view.rows[d]) for d in ra[np.concatenate([[True], ra[1:] != ra[:-1]])]]
    assert order == sorted(a_n)    # the A sequence the case was built for, in one chunk
    np.testing.assert_array_equal(eng.to_host(eng.launch_count(handle)).numpy(), want)
    base = _partials(eng, handle, 6)
    assert 63 in eng.ext.PAIR_VARIANTS
    for variant in eng.ext.PAIR_VARIANTS:
        np.testing.assert_array_equal(_partials(eng, handle, variant), base, err_msg=f"variant {variant}")
    # the product's own choice of kernel
    dflt = GpuEngine(dev)
    dflt.and2_cq = 64
    np.testing.assert_array_equal(dflt.count(exprs), want)
