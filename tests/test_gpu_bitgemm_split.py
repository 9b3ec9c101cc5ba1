"""bitgemm (bitgemm.hip) with one output matrix per K-split: the per-shard
count tables of the hot-pair table are one launch over a block of shards.
Every count is compared exactly with a numpy popcount of the same words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPLIT_WORDS = 16384      # one shard of densify output
SPLITS = 3


def _rows(rng, n):
    """n dense rows of SPLITS * SPLIT_WORDS words: mixed densities, an empty
    row, a full row, and bits on both sides of every split boundary."""
    kw = SPLITS * SPLIT_WORDS
    a = rng.integers(0, 1 << 63, size=(n, kw), dtype=np.int64, endpoint=False).view(np.uint64)
    a &= rng.integers(0, 1 << 63, size=(n, kw), dtype=np.int64, endpoint=False).view(np.uint64)
    a[::3] &= rng.integers(0, 1 << 63, size=(len(a[::3]), kw), dtype=np.int64).view(np.uint64)
    a[1] = 0
    a[2] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for y in range(1, SPLITS):
        a[3, y * SPLIT_WORDS - 1] = np.uint64(1) << np.uint64(63)
        a[3, y * SPLIT_WORDS] = np.uint64(1)
    return a


def _want(a, b):
    """int64[SPLITS][M][N] popcounts of a[m] & b[n] per split."""
    out = np.zeros((SPLITS, len(a), len(b)), np.int64)
    step = 1024   # words: 0/1 products summed in float32 over 65536 bits stay exact (< 2^24)
    for y in range(SPLITS):
        for k in range(y * SPLIT_WORDS, (y + 1) * SPLIT_WORDS, step):
            ab = np.unpackbits(np.ascontiguousarray(a[:, k:k + step]).view(np.uint8), axis=1).astype(np.float32)
            bb = ab if b is a else \
                np.unpackbits(np.ascontiguousarray(b[:, k:k + step]).view(np.uint8), axis=1).astype(np.float32)
            out[y] += (ab @ bb.T).astype(np.int64)
    return out


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(31)
    out = {}
    for n in (70, 130):
        a = _rows(rng, n)
        out[n] = (a, _want(a, a))
    return out


@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("n", [70, 130])
def test_per_split_outputs(cases, n, mode):
    import torch
    from pilosa_amd.ops.device import kernels

    ext = kernels()
    a, want = cases[n]
    dev = torch.device("cuda:0")
    ta = torch.from_numpy(a.view(np.int64).reshape(-1)).to(dev)
    kw = SPLITS * SPLIT_WORDS
    # one matrix per split, a guard matrix behind them
    c = torch.zeros((SPLITS + 1, n, n), dtype=torch.int32, device=dev)
    c[SPLITS] = -7
    ext.bitgemm(ta, ta, n, n, kw, SPLITS, mode, c.view(-1), n * n, False)
    got = c.cpu().numpy()
    np.testing.assert_array_equal(got[:SPLITS], want)
    assert (got[SPLITS] == -7).all()
    # stride 0: every split adds into the one matrix
    c0 = torch.zeros((n, n), dtype=torch.int32, device=dev)
    ext.bitgemm(ta, ta, n, n, kw, SPLITS, mode, c0.view(-1))
    np.testing.assert_array_equal(c0.cpu().numpy(), want.sum(axis=0))
    # tiles strictly below the diagonal skipped: (min, max) still holds every count
    cs = torch.zeros((SPLITS, n, n), dtype=torch.int32, device=dev)
    ext.bitgemm(ta, ta, n, n, kw, SPLITS, mode, cs.view(-1), n * n, True)
    gs = cs.cpu().numpy()
    iu = np.triu_indices(n)
    np.testing.assert_array_equal(gs[:, iu[0], iu[1]], want[:, iu[0], iu[1]])
    tile = 128 if mode == 2 else 64
    m, k = np.indices((n, n))
    below = (m // tile) > (k // tile)
    assert below.any() == (n > tile) and (gs[:, below] == 0).all()


def test_split_output_must_fit():
    import torch
    from pilosa_amd.ops.device import kernels

    ext = kernels()
    dev = torch.device("cuda:0")
    n, kw = 4, 2 * SPLIT_WORDS
    ta = torch.zeros(n * kw, dtype=torch.int64, device=dev)
    c = torch.zeros(2 * n * n - 1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        ext.bitgemm(ta, ta, n, n, kw, 2, 2, c, n * n, False)
    with pytest.raises(RuntimeError):
        ext.bitgemm(ta, ta, n, n, kw, 2, 2, torch.zeros(2 * n * n, dtype=torch.int32, device=dev), n * n - 1, False)
