#!/usr/bin/env python3
"""Percentile(field=, nth=) on the config-4 index: what a request costs on

  (a) the client-side emulation a user had to write before the call existed:
      the binary search issued as separate PQL requests (Count / Min / Max,
      one Executor.execute each);
  (b) Percentile on the generic path (the same search inside the executor);
  (c) Percentile on the device path (bsi_kth_init + one launch per bit).

The index is built as bench.py builds BASELINE config 4 (int field ``v``,
depth 20, half the columns hold a value in [-1000, 1e6]; set field ``g`` for
filters) and opened with a lazy holder.  Every timing is the host clock around
a call that ends in a device-to-host read; the three variants alternate
request by request in one process, after a warm-up of every shape.

    python scripts/percentile_bench.py --cols 1000000000 --reps 60 --out result.json
"""
import argparse
import json
import math
import os
import shutil
import statistics
import sys
import tempfile
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_index(base, cols, threads):
    from pilosa_amd import _roaring
    from pilosa_amd.models.field import FieldOptions
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.shardwidth import SHARD_WIDTH
    nshards = math.ceil(cols / SHARD_WIDTH)
    h = Holder(base).open()
    idx = h.create_index("c", track_existence=False)
    fv = idx.create_field("v", FieldOptions(type="int", min=-1000, max=1_000_000))
    fv.options.bit_depth = 20
    fv.bsi.bit_depth = 20
    fv.save_meta()
    idx.create_field("g", FieldOptions(cache_type="none"))
    h.close()

    def frag_dir(field, view):
        d = os.path.join(base, "c", field, "views", view, "fragments")
        os.makedirs(d, exist_ok=True)
        return d
    _roaring.write_bsi_fragments(frag_dir("v", "bsig_v"), 0, nshards, cols, 20, 0.5, -1000, 1_000_000, 7, threads)
    _roaring.write_zipf_fragments(frag_dir("g", "standard"), 0, nshards, cols, 1000, 1.0, 1.6, 50.0, 11, threads,
                                  cache_size=0)
    return list(range(nshards))


def client_side(ex, shards, filt, nth):
    """(a): the search of Executor._percentile as a client would issue it."""
    from pilosa_amd.executor import Executor

    def one(q):
        return ex.execute("c", q, shards=shards).results[0]
    consider = f"Intersect({filt}, Row(v != null))" if filt else "Row(v != null)"
    pre = filt + ", " if filt else ""
    n = one(f"Count({consider})")
    if n <= 0:
        return 0, 0
    k = Executor.percentile_rank(Fraction(nth), n)
    lo, hi = one(f"Min({pre}field=v)").val, one(f"Max({pre}field=v)").val
    while lo < hi:
        mid = (lo + hi) >> 1
        if one(f"Count(Intersect({consider}, Row(v <= {mid})))") >= k:
            hi = mid
        else:
            lo = mid + 1
    return lo, one(f"Count(Intersect({consider}, Row(v == {lo})))")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cols", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=60, help="timed requests per row and variant (>= 50 for a record)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--data-dir", default=None, help="keep / reuse the index here")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()

    import torch

    from pilosa_amd.executor import Executor
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.ops.gpu_executor import GpuExecutor

    own = args.data_dir is None
    base = tempfile.mkdtemp(prefix="pilosa_pct_") if own else os.path.join(args.data_dir, f"pct_{args.cols}")
    try:
        t0 = time.perf_counter()
        marker = os.path.join(base, ".ready")
        if not os.path.exists(marker):
            shutil.rmtree(base, ignore_errors=True)
            os.makedirs(base, exist_ok=True)
            build_index(base, args.cols, args.threads)
            open(marker, "w").close()
        from pilosa_amd.shardwidth import SHARD_WIDTH
        shards = list(range(math.ceil(args.cols / SHARD_WIDTH)))
        print(f"index ready: {len(shards)} shards ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
        holder = Holder(base, lazy_fragments=True).open()
        gpu = GpuExecutor(holder, "cuda:0")
        ex = Executor(holder, gpu=gpu)
        gpu.executor = ex
        ex.strict_gpu = True
        fast = gpu.bsi_percentile

        def decline(*a, **k):
            raise NotImplementedError

        def run_a(filt, nth):
            return client_side(ex, shards, filt, nth)

        def run_b(filt, nth):
            gpu.bsi_percentile = decline
            try:
                r = ex.execute("c", f"Percentile({filt + ', ' if filt else ''}field=v, nth={nth})",
                               shards=shards).results[0]
            finally:
                gpu.bsi_percentile = fast
            return r.val, r.count

        def run_c(filt, nth):
            n0 = gpu.percentile_device
            r = ex.execute("c", f"Percentile({filt + ', ' if filt else ''}field=v, nth={nth})",
                           shards=shards).results[0]
            assert gpu.percentile_device == n0 + 1, "the device path declined"
            return r.val, r.count

        variants = (("a_client_side", run_a), ("b_generic", run_b), ("c_device", run_c))
        rows = []
        for filt in ("", "Row(g=3)"):
            for nth in ("1", "50", "99.9"):
                answers = {}
                for name, fn in variants:
                    for _ in range(args.warmup):
                        answers[name] = fn(filt, nth)
                assert len(set(answers.values())) == 1, f"variants disagree: {answers}"
                ms = {name: [] for name, _ in variants}
                for _ in range(args.reps):
                    for name, fn in variants:     # alternating, request by request
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn(filt, nth)
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                row = {"filter": filt or None, "nth": nth, "value": answers["c_device"][0],
                       "count": answers["c_device"][1]}
                for name, _ in variants:
                    v = sorted(ms[name])
                    row[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4),
                                 "p10_ms": round(v[len(v) // 10], 4), "p90_ms": round(v[(len(v) * 9) // 10], 4),
                                 "max_ms": round(v[-1], 4)}
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        res = {"bench": "percentile", "cols": args.cols, "shards": len(shards), "depth": 20, "reps": args.reps,
               "device": torch.cuda.get_device_name(0), "rows": rows}
        ex.close()
        holder.close()
    finally:
        if own:
            shutil.rmtree(base, ignore_errors=True)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
