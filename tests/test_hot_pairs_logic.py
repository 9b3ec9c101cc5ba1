"""Host-side logic of the hot-pair table (ops/device.py): table size, which
batches may read it, which shards a write made stale, how shards are grouped
into build blocks, and the ViewDev record layout."""
import numpy as np

from pilosa_amd.ops.device import (VIEWDEV_DTYPE, hot_stale_shards, hot_table_passable, hot_table_rows, shard_runs)


def test_table_rows_caps():
    free = 200 << 30
    assert hot_table_rows(256, 1000, 954, free) == 256
    assert hot_table_rows(256, 100, 954, free) == 100          # no more rows than the view has
    assert hot_table_rows(0, 100, 954, free) == 0 and hot_table_rows(-1, 100, 954, free) == 0
    assert hot_table_rows(256, 0, 954, free) == 0 and hot_table_rows(256, 100, 0, free) == 0
    # a quarter of free memory: S * H * H * 4 bytes <= free / 4
    for S, fr in ((954, 1 << 30), (954, 100 << 20), (3, 4096), (1, 15), (1, 0)):
        h = hot_table_rows(1 << 20, 1 << 20, S, fr)
        assert S * h * h * 4 <= fr // 4
        assert S * (h + 1) * (h + 1) * 4 > fr // 4


def test_passable_only_at_the_synchronised_generation():
    assert hot_table_passable(3, 10, 3, 10)
    assert not hot_table_passable(3, 10, 3, 11)     # a write since the last synchronisation
    assert not hot_table_passable(3, 10, 4, 10)     # the dense row directory changed
    assert not hot_table_passable(3, 10, 4, 11)


def test_stale_shards():
    snap = np.array([0, 2, 5, 5], np.int64)
    assert hot_stale_shards(snap, snap.copy()).tolist() == []
    assert hot_stale_shards(snap, np.array([0, 3, 5, 9])).tolist() == [1, 3]
    assert hot_stale_shards(snap, snap + 1).tolist() == [0, 1, 2, 3]
    assert hot_stale_shards(snap, snap).dtype == np.int64


def test_shard_runs():
    assert shard_runs([], 4) == []
    assert shard_runs(np.arange(10), 4) == [(0, 4), (4, 8), (8, 10)]
    assert shard_runs([0, 1, 2, 5, 7, 8], 16) == [(0, 3), (5, 6), (7, 9)]
    assert shard_runs([3], 1) == [(3, 4)]
    assert shard_runs([3, 4, 5], 1) == [(3, 4), (4, 5), (5, 6)]
    runs = shard_runs(np.arange(954), 48)
    assert runs[0] == (0, 48) and runs[-1][1] == 954 and all(b - a <= 48 for a, b in runs)
    assert sum(b - a for a, b in runs) == 954


def test_viewdev_record_holds_the_table_fields():
    names = VIEWDEV_DTYPE.names
    assert names[-4:] == ("hot_counts", "hot_slot", "hot_valid", "hot_h")
    assert VIEWDEV_DTYPE.itemsize == 120 and VIEWDEV_DTYPE.fields["hot_counts"][1] == 88
