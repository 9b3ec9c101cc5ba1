"""Anti-entropy block checksums of one view: a full pass from the resident HBM
arena (GpuExecutor.block_checksums, kernels/sync_kernels.hip) against the
host path's best case, Fragment.blocks() over the same fragments already in
heap with their checksum caches cleared.  Then the cold case: the holder is
reopened lazily and each path hashes every fragment once, with the growth of
the process's resident set -- the host path reads every fragment into heap,
the device path streams the files into the arena.

    python scripts/blocks_bench.py --shards 64 --rows 1000 --fill 1000000
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rss_mb() -> float:
    with open("/proc/self/statm") as fh:
        return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--fill", type=int, default=1_000_000, help="bits per shard")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()

    import torch
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.ops.device import GpuEngine
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    from pilosa_amd.shardwidth import SHARD_WIDTH as SW
    rng = np.random.default_rng(0)
    d = tempfile.mkdtemp(prefix="pilosa_blocks_bench_", dir="/tmp")
    h = Holder(d).open()
    f = h.create_index("i").create_field("f")
    S = args.shards
    for s in range(S):
        rows = (rng.zipf(1.5, args.fill) % args.rows).astype(np.uint64)
        cols = (np.uint64(s * SW) + rng.integers(0, SW, args.fill).astype(np.uint64))
        f.import_bits(rows, cols)
    shards = tuple(range(S))
    frags = [f.view("standard").fragment(s) for s in shards]
    g = GpuExecutor(h, "cuda:0")
    dv = g.view_arena("i", "f", "standard", shards)
    torch.cuda.synchronize()
    out = {"shards": S, "rows": args.rows, "fill_bits_per_shard": args.fill}

    # device: memo cleared, so every (fragment, block) unit is hashed; the call
    # ends with the digests on the host (synchronised)
    dev_t = []
    for k in range(args.runs + 1):
        g._block_memo.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = g.block_checksums("i", "f", "standard", shards)
        if k:   # the first run warms the kernel
            dev_t.append(time.perf_counter() - t0)
    # host, best case: storage in heap, only the checksum cache cleared
    host_t = []
    for k in range(args.runs + 1):
        for fr in frags:
            fr.checksums.clear()
        t0 = time.perf_counter()
        want = {s: fr.blocks() for s, fr in zip(shards, frags)}
        if k:
            host_t.append(time.perf_counter() - t0)
    out["verified"] = got == want
    out["device_pass_s"] = round(statistics.median(dev_t), 5)
    out["device_pass_min_s"] = round(min(dev_t), 5)
    out["host_warm_pass_s"] = round(statistics.median(host_t), 5)
    out["host_warm_pass_min_s"] = round(min(host_t), 5)
    out["host_over_device"] = round(out["host_warm_pass_s"] / out["device_pass_s"], 2)
    # per-unit breakdown: the pass is as long as its slowest workgroups
    bids, d0, d1 = GpuEngine.block_ranges(dv)
    units = np.empty((S, len(bids), 3), np.int32)
    for s in range(S):
        units[s, :, 0], units[s, :, 1], units[s, :, 2] = s, d0, d1
    n, _ = g.engine.block_hash(dv, units.reshape(-1, 3))
    out["units"] = int(len(n))
    out["positions"] = int(n.sum())
    out["largest_unit_positions"] = int(n.max())
    out["device_positions_per_s"] = round(out["positions"] / out["device_pass_s"])
    out["host_positions_per_s"] = round(out["positions"] / out["host_warm_pass_s"])
    one = units.reshape(-1, 3)[int(np.argmax(n))]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.engine.block_hash(dv, one.reshape(1, 3))
    out["largest_unit_alone_s"] = round(time.perf_counter() - t0, 5)

    # cold fragments: each path hashes the lazily reopened holder once, in a
    # fresh process of its own (a heap that already held the fragments would
    # hide the growth)
    out["fragment_file_mb"] = round(sum(os.path.getsize(fr.path) for fr in frags) / 2**20, 1)
    del dv
    g.invalidate()
    h.close()
    digests = {}
    for path in ("device", "host"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cold-child", path, "--dir", d,
                            "--shards", str(S)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"cold {path} pass failed: {r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        digests[path] = res.pop("digest")
        out.update({f"cold_{path}_{k}": v for k, v in res.items()})
    out["verified_cold"] = digests["device"] == digests["host"]
    print(json.dumps(out))
    shutil.rmtree(d, ignore_errors=True)


def cold_child(path: str, d: str, S: int):
    """One pass over the lazily opened holder at ``d``: resident-set growth
    from just before the pass (the runtime is initialised by then)."""
    import hashlib

    from pilosa_amd.models.holder import Holder
    shards = tuple(range(S))
    h = Holder(d, lazy_fragments=True).open()
    frags = [h.fragment("i", "f", "standard", s) for s in shards]
    g = None
    if path == "device":
        import torch
        from pilosa_amd.ops.gpu_executor import GpuExecutor
        g = GpuExecutor(h, "cuda:0")
        torch.zeros(1, device="cuda:0")
        torch.cuda.synchronize()
    r0 = rss_mb()
    t0 = time.perf_counter()
    if g is not None:
        got = g.block_checksums("i", "f", "standard", shards)
    else:
        got = {s: fr.blocks() for s, fr in zip(shards, frags)}
    dt = time.perf_counter() - t0
    res = {"pass_s": round(dt, 4), "rss_before_mb": round(r0, 1), "rss_growth_mb": round(rss_mb() - r0, 1),
           "fragments_still_cold": sum(fr.is_cold() for fr in frags),
           "digest": hashlib.sha256(repr(sorted(got.items())).encode()).hexdigest()}
    print(json.dumps(res))
    h.close()


if __name__ == "__main__":
    if "--cold-child" in sys.argv:
        cp = argparse.ArgumentParser()
        cp.add_argument("--cold-child", choices=("device", "host"))
        cp.add_argument("--dir")
        cp.add_argument("--shards", type=int)
        a = cp.parse_args()
        cold_child(a.cold_child, a.dir, a.shards)
    else:
        main()
