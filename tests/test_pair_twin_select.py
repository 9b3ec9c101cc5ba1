"""Row selection for the pair kernel's bitmap twins (ops/device.py
select_twin_rows): plain numpy over a synthetic meta table."""
import numpy as np

from pilosa_amd.ops.device import select_twin_rows

ARR, BMP, RUN = 1, 2, 3


def _shard(rows):
    """rows: per dense row a list of (type, n) containers -> (rowptr, meta)."""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    meta = [j | (t << 4) | (n << 6) | (12345 << 23) for r in rows for j, (t, n) in enumerate(r)]
    return rp, np.asarray(meta, np.int64)


def test_picks_mostly_array_rows_with_mean_above_cutoff():
    rows = [
        [(ARR, 3000)] * 4,                       # 0: dense arrays -> picked
        [(BMP, 30000)] * 4,                      # 1: bitmaps already
        [(ARR, 2049), (ARR, 2048)],              # 2: mean 2048.5, just above 2048
        [(ARR, 2048), (ARR, 2048)],              # 3: mean == cutoff -> not above
        [(ARR, 4000), (BMP, 5000), (BMP, 5000)],  # 4: mostly bitmaps
        [(ARR, 4000), (BMP, 5000)],              # 5: exactly half arrays -> not "mostly"
        [(ARR, 4000), (ARR, 3000), (RUN, 60000)],  # 6: two of three arrays
        [],                                      # 7: absent row
        [(ARR, 10)] * 16,                        # 8: sparse
    ]
    got = select_twin_rows([_shard(rows)], len(rows), 2048, 64)
    assert got.dtype == np.int32 and got.tolist() == [0, 2, 6]
    assert select_twin_rows([_shard(rows)], len(rows), 3072, 64).tolist() == [6]
    assert select_twin_rows([_shard(rows)], len(rows), 4096, 64).tolist() == []


def test_sample_shards_add_up_and_row_limit_keeps_the_densest():
    a = [[(ARR, 4000)], [(ARR, 100)], [(ARR, 3500)] * 2, [(ARR, 2100)] * 3]
    b = [[(ARR, 100)], [(ARR, 4000)], [(ARR, 3500)] * 2, []]
    # rows 0 and 1: mean (4000 + 100) / 2 = 2050 over both shards
    assert select_twin_rows([_shard(a), _shard(b)], 4, 2048, 64).tolist() == [0, 1, 2, 3]
    assert select_twin_rows([_shard(a)], 4, 2048, 64).tolist() == [0, 2, 3]
    # array values per row: 4100, 4100, 14000, 6300 -> the two densest, sorted
    assert select_twin_rows([_shard(a), _shard(b)], 4, 2048, 2).tolist() == [2, 3]
    assert select_twin_rows([_shard(a), _shard(b)], 4, 2048, 0).tolist() == []
    assert select_twin_rows([], 4, 2048, 8).tolist() == []
