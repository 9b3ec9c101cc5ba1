#!/usr/bin/env python3
"""Extract(filter, Rows(field=)...): what a call costs on the device and on
the host.

The index is the profiles/distinct shape: --shards shards (64), two depth-20
int fields ``v`` and ``u`` whose planes are bitmap containers, half the columns
holding a value.  The filters are three rows of a set field ``s`` with about
1e3, 1e5 and 1e6 random columns over all shards (cases ``1e3``, ``1e5``,
``1e6``; PILOSA_EXTRACT_MAX_COLUMNS is raised to 2^21 for the run).

Reported per case, each a median over --reps runs with p10 / p90 / min / max:

  kernel    bsi_extract_kernel alone (device events around the launch; the
            count pass and the cumsum are done once, outside) for every n in
            --slots;
  sum       the bsi_sum launch over the same field and filter, the reference
            point: that kernel reads the same planes exactly once;
  count     the expr_count launch + cumsum + the one read of the total (the
            offsets step of a request);
  device    the request through Executor.execute on the device route, with one
            int field and with two;
  host      the same requests with PILOSA_EXTRACT_DEVICE=0 (--host-reps runs).

    python scripts/extract_bench.py --out extract_bench.json
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
CASES = {"1e3": (1, 1_000), "1e5": (2, 100_000), "1e6": (3, 1_000_000)}


def build_index(base, nshards, threads):
    import numpy as np

    from pilosa_amd import _roaring
    from pilosa_amd.models.field import FieldOptions
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.shardwidth import SHARD_WIDTH
    cols = nshards * SHARD_WIDTH
    h = Holder(base).open()
    idx = h.create_index("c", track_existence=False)
    for name in ("v", "u"):
        f = idx.create_field(name, FieldOptions(type="int", min=-1000, max=1_000_000))
        f.options.bit_depth = DEPTH
        f.bsi.bit_depth = DEPTH
        f.save_meta()
    s = idx.create_field("s", FieldOptions(cache_type="none"))
    rng = np.random.default_rng(13)
    for row, n in CASES.values():
        c = np.unique(rng.integers(0, cols, n, dtype=np.uint64))
        s.import_bits(np.full(len(c), row, np.uint64), c)
    h.close()
    for seed, name in ((7, "v"), (9, "u")):
        d = os.path.join(base, "c", name, "views", "bsig_" + name, "fragments")
        os.makedirs(d, exist_ok=True)
        _roaring.write_bsi_fragments(d, 0, nshards, cols, DEPTH, 0.5, -1000, 1_000_000, seed, threads)


def stats(ms):
    v = sorted(ms)
    return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(v[len(v) // 10], 4),
            "p90_ms": round(v[(len(v) * 9) // 10], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="1e3,1e5,1e6")
    ap.add_argument("--shards", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slots", default="1,2,4,8")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from pilosa_amd import shardwidth
    from pilosa_amd.executor import Executor
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.ops.device import flat_mask
    from pilosa_amd.ops.gpu_executor import EMPTY, GpuExecutor, extract_slots_env
    from pilosa_amd.pql import parse_string

    os.environ["PILOSA_EXTRACT_MAX_COLUMNS"] = str(1 << 21)
    base = tempfile.mkdtemp(prefix="pilosa_extract_")
    res = {"bench": "extract", "shards": args.shards, "depth": DEPTH, "reps": args.reps,
           "host_reps": args.host_reps, "cases": {}}
    try:
        t0 = time.perf_counter()
        build_index(base, args.shards, args.threads)
        shards = list(range(args.shards))
        print(f"index ready ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
        holder = Holder(base).open()
        gpu = GpuExecutor(holder, "cuda:0")
        ex = Executor(holder, gpu=gpu)
        gpu.executor = ex
        ex.strict_gpu = True
        eng = gpu.engine
        res["device"] = torch.cuda.get_device_name(0)
        res["request_slots"] = int(eng.ext.extract_slots(DEPTH, extract_slots_env()))

        def ev_time(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            return (time.perf_counter() - t) * 1e3, r

        def median_of(fn, reps, timer=ev_time):
            ms = []
            for i in range(args.warmup + reps):
                t = timer(fn)
                if i >= args.warmup:
                    ms.append(t)
            return stats(ms)

        bv = gpu.view_arena("c", "v", "bsig_v", shards)
        targs = torch.from_numpy(eng.bsi_args(bv, DEPTH))
        col_base = torch.from_numpy(np.asarray(bv.shards, dtype=np.int64) * shardwidth.ARENA_WIDTH).to(eng.device)
        for case in args.cases.split(","):
            row, _ = CASES[case]
            filt_text = f"Row(s={row})"
            out = {"filter": filt_text}
            filt = gpu.plan("c", parse_string(filt_text).calls[0], shards)
            assert filt is not EMPTY
            progs, ordered = eng._bsi_filter_program([filt], bv)
            tp, tv = eng.upload_batch(progs, ordered)
            S = bv.S
            mode = 2 if bool(flat_mask(progs).all()) else 0
            state = {}

            def count_step():
                counts = torch.zeros(S * 16, dtype=torch.int32, device=eng.device)
                eng.ext.expr_count(tp, tv, S, torch.empty(0, dtype=torch.int64, device=eng.device), counts, mode)
                c64 = counts.to(torch.int64)
                ends = torch.cumsum(c64, 0)
                state["off"] = torch.where(c64 > 0, ends - c64, torch.full_like(ends, -1)).contiguous()
                state["total"] = int(eng.to_host(ends[-1:]).item())

            out["count"] = median_of(count_step, args.reps, lambda fn: timed(fn)[0])
            total = state["total"]
            out["columns"] = total
            columns = torch.empty(total, dtype=torch.int64, device=eng.device)
            values = torch.empty(total, dtype=torch.int64, device=eng.device)
            valid = torch.empty(total, dtype=torch.uint8, device=eng.device)
            out["kernel"] = []
            want = None
            for n in [int(x) for x in args.slots.split(",")]:
                used = int(eng.ext.extract_slots(DEPTH, n))
                if used != n:
                    out["kernel"].append({"slots": n, "clamped_to": used})
                    continue

                def launch():
                    eng.ext.bsi_extract(tp, tv, S, targs, n, state["off"], col_base, -1000, columns, values, valid)
                row_ = {"slots": n, **median_of(launch, args.reps)}
                got = (int(columns.sum()), int(values.sum()), int(valid.sum()))   # a cheap fingerprint
                want = want or got
                assert got == want, f"slot counts disagree: {n}"
                out["kernel"].append(row_)
                print(json.dumps({case: row_}), file=sys.stderr, flush=True)
            out["sum"] = median_of(lambda: eng.bsi_sum_async([filt], bv, DEPTH, matrix=False), args.reps)

            # ---- request level: device route, then the host path on the same index
            for label, fields in (("one_field", ("v",)), ("two_fields", ("v", "u"))):
                q = f"Extract({filt_text}, " + ", ".join(f"Rows(field={f})" for f in fields) + ")"
                os.environ["PILOSA_EXTRACT_DEVICE"] = "1"
                box = {}

                def dev():
                    n0 = gpu.extract_device
                    box["dev"] = ex.execute("c", q, shards=shards).results[0]
                    assert gpu.extract_device == n0 + len(fields), "the device route declined"
                out[label] = {"query": q, "device_request": median_of(dev, args.reps, lambda fn: timed(fn)[0])}
                os.environ["PILOSA_EXTRACT_DEVICE"] = "0"

                def host():
                    n0 = gpu.extract_device
                    box["host"] = ex.execute("c", q, shards=shards).results[0]
                    assert gpu.extract_device == n0
                ms = [timed(host)[0] for _ in range(args.host_reps)]
                out[label]["host_request"] = stats(ms)
                assert box["dev"] == box["host"] and len(box["dev"]) == total, "device and host answers differ"
                os.environ["PILOSA_EXTRACT_DEVICE"] = "1"
                print(json.dumps({case: {label: out[label]}}), file=sys.stderr, flush=True)
            res["cases"][case] = out
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
