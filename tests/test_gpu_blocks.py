"""Anti-entropy from HBM (K22, kernels/sync_kernels.hip): block checksums and
block data read from the device arena equal the host path byte for byte --
``Fragment.blocks()`` / ``block_data()``, or XXH64 (``xxhash``) over the
fragment's positions grouped by 100-row block -- and leave cold fragments cold.
Every test runs at the process's shard width; the last one re-runs this file
at 2^16, 2^18 and 2^22 columns."""
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import xxhash

from pilosa_amd import _roaring as R
from pilosa_amd import shardwidth
from tests.helpers import SW, Env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = np.uint64(100 * SW)
CPR = SW >> 16          # containers per row


def P(row, col):
    """Positions row * ShardWidth + col (col: int or array)."""
    return np.uint64(row) * np.uint64(SW) + np.asarray(col, dtype=np.uint64)


def _host_blocks(bm):
    """The reference semantics written out: XXH64 over each 100-row block's
    positions in ascending order, 8 big-endian bytes each."""
    vals = bm.slice() if bm is not None else np.zeros(0, np.uint64)
    out = []
    for bid in np.unique(vals // BLOCK).tolist():
        part = vals[vals // BLOCK == np.uint64(bid)]
        out.append((int(bid), xxhash.xxh64(part.astype(">u8").tobytes()).digest()))
    return out


def _arena(bitmaps, patchable=False):
    """Device arena of host fragments (one bitmap per shard, None = missing)."""
    import torch
    from pilosa_amd.ops.device import DeviceView
    M = shardwidth.DEVICE_SUBSHARDS
    if shardwidth.WIDE:
        bitmaps = [b.sub_shard(shardwidth.KEY_SHIFT, i) if b is not None else None
                   for b in bitmaps for i in range(M)]
    return DeviceView.from_bitmaps(list(bitmaps), torch.device("cuda:0"),
                                   shards=shardwidth.device_shards(range(len(bitmaps) // M)), patchable=patchable)


@pytest.fixture(scope="module")
def engine():
    import torch
    from pilosa_amd.ops.device import GpuEngine
    return GpuEngine(torch.device("cuda:0"))


def _device_blocks(engine, dv, nfrags):
    """[(block id, digest)] per fragment, all fragments in one launch."""
    bids, d0, d1 = engine.block_ranges(dv)
    B, M = len(bids), shardwidth.DEVICE_SUBSHARDS
    units = np.empty((nfrags, B, 3), np.int32)
    for f in range(nfrags):
        units[f, :, 0], units[f, :, 1], units[f, :, 2] = f * M, d0, d1
    n, h = engine.block_hash(dv, units.reshape(-1, 3))
    dig = h.astype(">u8").tobytes()
    return [[(int(bids[b]), dig[8 * (f * B + b):8 * (f * B + b) + 8]) for b in range(B) if n[f * B + b]]
            for f in range(nfrags)], n.reshape(nfrags, B)


def _check(engine, frags):
    dv = _arena(frags)
    got, n = _device_blocks(engine, dv, len(frags))
    for f, bm in enumerate(frags):
        assert got[f] == _host_blocks(bm), f"fragment {f}"
    return dv, n


def _straddle_positions(first_row):
    """3 + 2 + 1 + 6 bits: two containers of one row (one, at 2^16 columns),
    then two consecutive rows -- every stripe of 4 crosses a boundary."""
    r = first_row
    if CPR > 1:
        a = [P(r, [5, 70, 65535]), P(r, [65536 + 1, 65536 + 9])]
    else:
        a = [P(r, [5, 70, 65535]), P(r + 1, [1, 9])]
        r += 1
    return np.concatenate(a + [P(r + 1, [77]), P(r + 2, [0, 1, 2, 3, 500, 65535])])


def test_finalisation_lengths_and_omitted_block(engine):
    """Blocks of exactly 1..9 positions (short path, merge, 0..3 tail rounds);
    block 9 exists in the row directory only through the second fragment, so
    the first must omit it."""
    rng = np.random.default_rng(1)
    pos = [P(100 * (k - 1) + int(rng.integers(0, 100)), np.sort(rng.choice(SW, k, replace=False)))
           for k in range(1, 10)]
    a = R.Bitmap(np.concatenate(pos))
    b = R.Bitmap(P(950, [3, 4]))
    dv, n = _check(engine, [a, b])
    assert n[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 0] and n[1].tolist() == [0] * 9 + [2]


def test_stripes_straddle_containers_and_rows(engine):
    a = R.Bitmap(_straddle_positions(200))
    _, n = _check(engine, [a])
    assert n.tolist() == [[12]]
    # three fragments: units of different fragments share one launch
    frags = [R.Bitmap(_straddle_positions(200)), R.Bitmap(_straddle_positions(300)),
             R.Bitmap(np.concatenate([_straddle_positions(200), P(399, [8])]))]
    _, n = _check(engine, frags)
    assert n.sum(axis=1).tolist() == [12, 12, 13]
    if shardwidth.WIDE:
        # 3 positions end arena sub-shard 0 of a row, 2 begin sub-shard 1, 1 sits in
        # the last sub-shard, 6 in the next row: stripes cross sub-shard boundaries
        M, sub = shardwidth.DEVICE_SUBSHARDS, 1 << 20
        a = R.Bitmap(np.concatenate([P(200, [sub - 70000, sub - 2, sub - 1]), P(200, [sub, sub + 65536]),
                                     P(200, [(M - 1) * sub + 5]), P(201, [0, 1, sub - 1, sub, 2 * sub, SW - 1])]))
        _, n = _check(engine, [a, R.Bitmap(P(200, [sub - 1, sub]))])
        assert n.tolist() == [[12], [2]]


def test_every_encoding_and_edge(engine):
    rng = np.random.default_rng(2)
    rows = [
        P(0, [12345]),                                                   # array of 1
        P(1, np.sort(rng.choice(65536, 4096, replace=False))),           # array of 4096
        P(2, np.sort(rng.choice(65536, 4097, replace=False))),           # bitmap of 4097
        P(3, np.arange(65536)),                                          # full container
        P(4, np.arange(65536)),                                          # ... as one run
        P(5, (np.arange(3000) * 20)[:, None] + np.arange(7)[None, :]),   # many short runs
        P(6, [0, 65535]),                                                # lowest and highest value
        P(7, (np.arange(CPR) * 65536)[:, None] + rng.choice(65536, 5, replace=False)[None, :]),  # every key
    ]
    plain = R.Bitmap(np.unique(np.concatenate([r.ravel() for r in rows])))
    opt = plain.clone()
    opt.optimize()                      # rows 4 and 5 (and 3) become run containers
    kinds = {t for _, t, _ in opt.container_info()} | {t for _, t, _ in plain.container_info()}
    assert {"array", "bitmap", "run"} <= kinds
    _check(engine, [plain, opt])


def _random_fragment_here(rng, nrows):
    from tests.test_gpu_kernels import _random_fragment
    bm = _random_fragment(rng, nrows=nrows)
    if SW == 1 << 20:
        return bm
    p = bm.slice()      # the fixture is written for 2^20 columns: fold / spread it to this width
    bm = R.Bitmap(np.unique((p >> np.uint64(20)) * np.uint64(SW) + (p & np.uint64((1 << 20) - 1)) % np.uint64(SW)))
    bm.optimize()
    return bm


def test_random_fragments_all_container_kinds(engine):
    rng = np.random.default_rng(3)
    _check(engine, [_random_fragment_here(rng, 8), None, _random_fragment_here(rng, 5)])


def test_block_boundaries_and_64_bit_rows(engine):
    big = 2**40 + 3
    a = R.Bitmap(np.concatenate([P(r, [1, 2, SW - 1]) for r in (99, 100, 199, 200)] + [P(big, [7, SW - 2])]))
    dv, n = _check(engine, [a])
    bids, _, _ = engine.block_ranges(dv)
    assert bids.tolist() == [0, 1, 2, big // 100] and n.tolist() == [[3, 6, 3, 2]]


def _executor_env():
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    env = Env(gpu=lambda h: GpuExecutor(h, "cuda:0"))
    env.create_index("i")
    env.field("i", "g")
    env.executor.gpu.executor = env.executor
    return env


def _frag_blocks(env, shards):
    return {s: env.holder.fragment("i", "g", "standard", s).blocks() for s in shards}


def test_checksums_after_device_writes_and_compaction(engine):
    """Sets and clears replayed into the arena (a cleared-out container leaves
    a dead metadata slot), then payload compaction: the checksums follow the
    fragments, and the arena was built once."""
    shards = (0, 1, 2)
    env = _executor_env()
    try:
        f = env.holder.index("i").field("g")
        g = env.executor.gpu
        rng = np.random.default_rng(5)
        for r in (0, 1, 2, 150, 151, 320):
            c = rng.choice(3 * SW, 3000, replace=False).astype(np.uint64)
            f.import_bits(np.full(len(c), r, np.uint64), c)
        whole = np.uint64(SW) + np.arange(min(SW, 65536), dtype=np.uint64)       # row 7's first container, shard 1
        f.import_bits(np.full(len(whole), 7, np.uint64), whole)
        assert g.block_checksums("i", "g", "standard", shards) == _frag_blocks(env, shards)
        l0 = g.launches
        assert g.block_checksums("i", "g", "standard", shards) == _frag_blocks(env, shards)
        assert g.launches == l0, "unchanged fragments are answered from the memo"
        f.import_bits(np.full(len(whole), 7, np.uint64), whole, clear=True)      # empties that container
        c = rng.choice(3 * SW, 4000, replace=False).astype(np.uint64)
        f.import_bits(np.full(len(c), 150, np.uint64), c)
        f.import_bits(np.full(2000, 1, np.uint64), c[:2000], clear=True)
        env.q("i", f"Set({SW + 11}, g=410) Clear({int(c[0])}, g=150)")
        assert g.block_checksums("i", "g", "standard", shards) == _frag_blocks(env, shards)
        assert g.rebuilds == 1
        dv = g.view_arena("i", "g", "standard", shards)
        if dv.garbage_u16:
            assert dv.compact()
        got, _ = _device_blocks(engine, dv, len(shards))
        assert {s: got[k] for k, s in enumerate(shards)} == _frag_blocks(env, shards)
        g.invalidate()
        assert g._block_memo == {}
        assert g.block_checksums("i", "g", "standard", (0, 1, 2, 9))[9] == []     # a missing fragment
    finally:
        env.close()


def test_block_data_equals_host():
    shards = (0, 1)
    env = _executor_env()
    try:
        f = env.holder.index("i").field("g")
        g = env.executor.gpu
        rng = np.random.default_rng(6)
        for r in (3, 99, 100, 101, 199, 250):
            c = rng.choice(2 * SW, 20000 if r == 100 else 700, replace=False).astype(np.uint64)
            f.import_bits(np.full(len(c), r, np.uint64), c)
        dense = np.uint64(SW) + np.arange(min(SW, 50000), dtype=np.uint64)
        f.import_bits(np.full(len(dense), 120, np.uint64), dense)
        for s in shards:
            frag = env.holder.fragment("i", "g", "standard", s)
            for block in (0, 1, 2):
                want = frag.block_data(block)
                l0 = g.launches
                got = g.block_data("i", "g", "standard", shards, s, block)
                assert g.launches > l0
                assert got[0].dtype == got[1].dtype == np.uint64 and len(want[0])
                assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
            for block in (3, 17):       # no rows in the directory / no data
                r, c = g.block_data("i", "g", "standard", shards, s, block)
                assert len(r) == len(c) == 0
    finally:
        env.close()


# ------------------------------------------------------------------ product path

def _populate_dir():
    """A data dir holding index i / field f over 4 shards, written through a
    host holder and closed."""
    from pilosa_amd.models.holder import Holder
    d = tempfile.mkdtemp()
    h = Holder(d).open()
    try:
        f = h.create_index("i").create_field("f")
        rng = np.random.default_rng(8)
        for shard in range(4):
            rows = np.concatenate([rng.integers(0, 350, 5000), np.full(3000, 120)])
            cols = shard * SW + np.concatenate([rng.integers(0, SW, 5000), rng.choice(SW, 3000, replace=False)])
            f.import_bits(rows.astype(np.uint64), cols.astype(np.uint64))
    finally:
        h.close()
    return d


def _open(d, gpu, **kw):
    from pilosa_amd.server.server import Server
    from pilosa_amd.utils.logger import CaptureLogger
    return Server(d, bind="127.0.0.1:0", gpu=gpu, logger=CaptureLogger(), **kw).open()


def test_api_answers_from_the_arena_and_fragments_stay_cold():
    from pilosa_amd.server.api import QueryRequest
    d = _populate_dir()
    d2 = d + "_host"
    shutil.copytree(d, d2)
    dev, host = _open(d, "on", lazy_fragments=True), _open(d2, "off")
    try:
        g = dev.executor.gpu
        assert g is not None and dev.executor.mesh is None
        frags = [dev.holder.fragment("i", "f", "standard", s) for s in range(4)]
        assert all(fr.is_cold() for fr in frags)
        for s in range(4):
            assert dev.api.fragment_blocks("i", "f", "standard", s) == host.api.fragment_blocks("i", "f", "standard", s)
        for s in range(4):
            for block in (0, 1, 3, 8):
                got = dev.api.fragment_block_data("i", "f", "standard", s, block)
                want = host.api.fragment_block_data("i", "f", "standard", s, block)
                assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
        assert all(fr.is_cold() for fr in frags), "anti-entropy reads must not materialise fragments"
        assert g.cold_loads == 1 and g.rebuilds == 1
        l0 = g.launches
        again = [dev.api.fragment_blocks("i", "f", "standard", s) for s in range(4)]
        assert g.launches == l0, "unchanged fragments launch nothing"
        # one Set: only its shard is hashed again, and its block follows
        before = {s: g._block_memo[("i", "f", "standard", s)][1] for s in range(4)}
        for srv in (dev, host):
            srv.api.query(QueryRequest(index="i", query=f"Set({2 * SW + 77}, f=215)"))
        l1 = g.launches
        got = dev.api.fragment_blocks("i", "f", "standard", 2)
        assert got == host.api.fragment_blocks("i", "f", "standard", 2)
        assert got != again[2] and [b["id"] for b in got if b not in again[2]] == [2]
        assert g.launches == l1 + 1 and g.rebuilds == 1
        for s in (0, 1, 3):
            assert g._block_memo[("i", "f", "standard", s)][1] is before[s]
            assert dev.api.fragment_blocks("i", "f", "standard", s) == again[s]
        assert g.launches == l1 + 1
    finally:
        dev.close()
        host.close()
        shutil.rmtree(d, ignore_errors=True)
        shutil.rmtree(d2, ignore_errors=True)


def _restart_holder_cold(srv):
    """The node's holder closed and reopened lazily, as after a restart: every
    fragment is cold again and no arena is resident."""
    from pilosa_amd.models.holder import Holder
    srv.holder.close()
    srv.holder = Holder(srv.data_dir, lazy_fragments=True).open()
    srv.executor.holder = srv.gpu.holder = srv.holder
    srv.gpu.invalidate()


def test_anti_entropy_repairs_from_the_device_and_keeps_the_rest_cold():
    """Two replicas of every shard, the local node on the GPU with cold
    fragments; the peer holds one bit the local node lacks (as in
    tests/test_server.py test_replication_and_failover)."""
    from pilosa_amd.parallel.cluster import URI
    d0 = _populate_dir()
    d1 = _populate_dir()
    kw = dict(replica_n=2, probe_interval=0.2, hasher="mod")
    from pilosa_amd.server.server import Server
    from pilosa_amd.utils.logger import CaptureLogger
    s0 = Server(d0, bind="127.0.0.1:0", node_id="node0", gpu="on", lazy_fragments=True, hosts=[], coordinator=True,
                logger=CaptureLogger(), **kw)
    s0.hosts = [URI.parse("127.0.0.1:1")]   # enable the membership loop
    s0.open()
    s1 = Server(d1, bind="127.0.0.1:0", node_id="node1", gpu="off", coordinator=False,
                coordinator_uri=s0.uri.normalize(), logger=CaptureLogger(), **kw).open()
    try:
        deadline = time.time() + 10
        while time.time() < deadline and not all(len(s.cluster.nodes) == 2 and s.cluster.state == "NORMAL"
                                                 for s in (s0, s1)):
            time.sleep(0.05)
        assert all(len(s.cluster.nodes) == 2 and s.cluster.state == "NORMAL" for s in (s0, s1))
        # (the join streamed fragments between the nodes, which reads them on the host)
        assert s1.holder.fragment("i", "f", "standard", 1).set_bit(230, SW + 4242)   # a new bit
        _restart_holder_cold(s0)
        frags = {s: s0.holder.fragment("i", "f", "standard", s) for s in range(4)}
        assert all(fr.is_cold() for fr in frags.values())
        g = s0.executor.gpu
        l0 = g.launches
        assert s0.sync_holder() is True
        assert g.launches > l0
        assert frags[1].bit(230, SW + 4242) is True
        assert frags[1].row_count(230) == s1.holder.fragment("i", "f", "standard", 1).row_count(230)
        assert all(frags[s].is_cold() for s in (0, 2, 3)), "fragments that did not differ stay cold"
        assert s0.api.fragment_blocks("i", "f", "standard", 1) == s1.api.fragment_blocks("i", "f", "standard", 1)
    finally:
        s0.close()
        s1.close()
        shutil.rmtree(d0, ignore_errors=True)
        shutil.rmtree(d1, ignore_errors=True)


# ------------------------------------------------------------------ other shard widths

@pytest.mark.timeout(600)
@pytest.mark.parametrize("exp", [16, 18, 22])
def test_blocks_at_other_shard_widths(exp):
    """The tests above at 2^16, 2^18 and 2^22 columns in a fresh interpreter
    (the width is fixed per process).  At 2^22 a shard is 4 arena sub-shards
    and the straddling test adds stripes that cross sub-shard boundaries."""
    env = dict(os.environ, PILOSA_SHARD_WIDTH=str(exp))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "--timeout", "300", "--timeout-method", "thread", "-k", "not other_shard_widths",
                        "tests/test_gpu_blocks.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=580)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1]
    assert "9 passed" in last and "skipped" not in last, r.stdout[-1000:]
