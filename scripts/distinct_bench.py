#!/usr/bin/env python3
"""Distinct(field=): what a call costs on the device and on the host.

One case per process invocation (--case):

  low       int field ``lo``: about 100 distinct values spread over the 2^20
            range, so every column finds its value already marked;
  high      int field ``v``: values uniform over [-1000, 1e6];
  filtered  ``v`` under the filter Row(g=3).

The index is the profiles/groupby_sum shape: --shards shards (64), depth-20
int fields whose planes are bitmap containers, half the columns holding a
value; ``g`` is a Zipf set field.  ``lo`` is imported for one shard and that
fragment file copied to the others (the kernel's work per shard is the same
and the import of 64 shards would take over a minute).

Reported, each a median over --reps runs:

  kernel    bsi_distinct_kernel alone (device events around the launch, the two
            bitmaps zeroed before each run) for every n in --slots and every
            marking variant in --marks;
  sum       the bsi_sum launch over the same field and filter, the reference
            point: that kernel reads the same planes exactly once;
  device    the request through Executor.execute on the device route;
  host      the same request with PILOSA_DISTINCT_DEVICE=0 (--host-reps runs).

    python scripts/distinct_bench.py --case low --out low.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEPTH = 20
CASES = {"low": ("lo", ""), "high": ("v", ""), "filtered": ("v", "Row(g=3)")}


def build_index(base, nshards, threads, case):
    import numpy as np

    from pilosa_amd import _roaring
    from pilosa_amd.models.field import FieldOptions
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.shardwidth import SHARD_WIDTH
    cols = nshards * SHARD_WIDTH
    field = CASES[case][0]
    h = Holder(base).open()
    idx = h.create_index("c", track_existence=False)
    f = idx.create_field(field, FieldOptions(type="int", min=-1000, max=1_000_000))
    if field == "lo":
        rng = np.random.default_rng(5)
        pool = np.unique(rng.integers(-1000, 1_000_001, 100))
        c = np.sort(rng.choice(SHARD_WIDTH, SHARD_WIDTH // 2, replace=False)).astype(np.uint64)
        f.import_values(c, pool[rng.integers(0, len(pool), len(c))])
        assert f.bsi.bit_depth == DEPTH
    else:
        f.options.bit_depth = DEPTH
        f.bsi.bit_depth = DEPTH
        f.save_meta()
    idx.create_field("g", FieldOptions(cache_type="none"))
    h.close()

    def frag_dir(name, view):
        d = os.path.join(base, "c", name, "views", view, "fragments")
        os.makedirs(d, exist_ok=True)
        return d
    if field == "lo":
        d = frag_dir("lo", "bsig_lo")
        for s in range(1, nshards):
            shutil.copyfile(os.path.join(d, "0"), os.path.join(d, str(s)))
    else:
        _roaring.write_bsi_fragments(frag_dir("v", "bsig_v"), 0, nshards, cols, DEPTH, 0.5, -1000, 1_000_000, 7, threads)
    if CASES[case][1]:
        _roaring.write_zipf_fragments(frag_dir("g", "standard"), 0, nshards, cols, 1000, 1.0, 1.6, 50.0, 11, threads,
                                      cache_size=0)


def stats(ms):
    v = sorted(ms)
    return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(v[len(v) // 10], 4),
            "p90_ms": round(v[(len(v) * 9) // 10], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--shards", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slots", default="1,2,4,8")
    ap.add_argument("--marks", default="0,1,2")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from pilosa_amd.executor import Executor
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.ops.gpu_executor import EMPTY, GpuExecutor
    from pilosa_amd.pql import parse_string

    field, filt_text = CASES[args.case]
    query = f"Distinct({filt_text + ', ' if filt_text else ''}field={field})"
    base = tempfile.mkdtemp(prefix="pilosa_distinct_")
    res = {"bench": "distinct", "case": args.case, "query": query, "shards": args.shards, "depth": DEPTH,
           "reps": args.reps, "host_reps": args.host_reps}
    try:
        t0 = time.perf_counter()
        build_index(base, args.shards, args.threads, args.case)
        shards = list(range(args.shards))
        print(f"index ready ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
        holder = Holder(base).open()
        gpu = GpuExecutor(holder, "cuda:0")
        ex = Executor(holder, gpu=gpu)
        gpu.executor = ex
        ex.strict_gpu = True
        eng = gpu.engine
        res["device"] = torch.cuda.get_device_name(0)

        def one(q):
            return ex.execute("c", q, shards=shards).results[0]

        def flat(r):
            return r.pos.columns().tolist(), r.neg.columns().tolist()

        # ---- kernel level
        bv = gpu.view_arena("c", field, "bsig_" + field, shards)
        filt = None
        if filt_text:
            filt = gpu.plan("c", parse_string(filt_text).calls[0], shards)
            assert filt is not EMPTY
        progs, ordered = eng._bsi_filter_program([filt], bv)
        targs = torch.from_numpy(eng.bsi_args(bv, DEPTH))
        tp, tv = eng.upload_batch(progs, ordered)
        words = (1 << DEPTH) >> 6
        bm = torch.zeros(2 * words, dtype=torch.int64, device=eng.device)

        def ev_time(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        want = None
        res["kernel"] = []
        for n in [int(x) for x in args.slots.split(",")]:
            used = int(eng.ext.distinct_slots(DEPTH, n))
            if used != n:
                res["kernel"].append({"slots": n, "clamped_to": used})
                continue
            for mark in [int(x) for x in args.marks.split(",")]:
                def launch():
                    eng.ext.bsi_distinct(tp, tv, bv.S, targs, n, mark, bm[:words], bm[words:])
                ms = []
                for i in range(args.warmup + args.reps):
                    bm.zero_()
                    t = ev_time(launch)
                    if i >= args.warmup:
                        ms.append(t)
                got = (int(torch.count_nonzero(bm[:words])), int(torch.count_nonzero(bm[words:])),
                       int(bm.sum()))     # a cheap fingerprint of the two bitmaps
                want = want or got
                assert got == want, f"variants disagree: slots {n} mark {mark}"
                row = {"slots": n, "mark": mark, **stats(ms)}
                res["kernel"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        # ---- the reference point: bsi_sum over the same field and filter
        ms = []
        for i in range(args.warmup + args.reps):
            t = ev_time(lambda: eng.bsi_sum_async([filt], bv, DEPTH, matrix=False))
            if i >= args.warmup:
                ms.append(t)
        res["sum"] = stats(ms)
        print(json.dumps({"sum": res["sum"]}), file=sys.stderr, flush=True)

        # ---- request level: device route, then the host path on the same index
        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            return (time.perf_counter() - t) * 1e3, r

        os.environ["PILOSA_DISTINCT_DEVICE"] = "1"
        ms = []
        for i in range(args.warmup + args.reps):
            n0 = gpu.distinct_device
            t, dev = timed(lambda: one(query))
            assert gpu.distinct_device == n0 + 1, "the device route declined"
            if i >= args.warmup:
                ms.append(t)
        res["device_request"] = stats(ms)
        from pilosa_amd.ops.gpu_executor import distinct_slots_env
        res["request_slots"] = int(eng.ext.distinct_slots(DEPTH, distinct_slots_env()))
        os.environ["PILOSA_DISTINCT_DEVICE"] = "0"
        ms = []
        for i in range(args.host_reps):
            n0 = gpu.distinct_device
            t, host = timed(lambda: one(query))
            assert gpu.distinct_device == n0
            ms.append(t)
        res["host_request"] = stats(ms)
        assert flat(dev) == flat(host), "device and host answers differ"
        res["distinct_values"] = len(flat(dev)[0]) + len(flat(dev)[1])
        ex.close()
        holder.close()
    finally:
        shutil.rmtree(base, ignore_errors=True)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
