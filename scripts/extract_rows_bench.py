#!/usr/bin/env python3
"""Extract(filter, Rows(field=)...) for set-like fields: rows_extract_kernel
(K28) against the host function, and where the device time goes.

The index: --shards shards (64) of the Zipf generator the other profiles use
(s = 1.6, v = 50, seed 1).  Set fields r64, r1000 and r50000 with 64, 1,000 and
50,000 rows at min(8, rows / 16) bits per column (the profiles/topk shapes) and
a mutex field mx (64 rows, one bit per column on average: the generator does
not keep the mutex invariant, a column holds up to several rows, and both
routes answer with the smallest).  The filters are three rows of
a set field ``s`` with about 1e3, 1e5 and 1e6 random columns over all shards
(PILOSA_EXTRACT_MAX_COLUMNS is raised to 2^21 for the run).

Reported per (field, filter), medians over --reps runs with p10 / p90:

  device   the request Extract(Row(s=k), Rows(field=F)) through
           Executor.execute with PILOSA_EXTRACT_ROWS_DEVICE=1 (host clock around
           the call; it ends with the copies to the host);
  host     the same request with PILOSA_EXTRACT_ROWS_DEVICE=0 -- the host
           function, which this kernel does not change (--host-reps runs, one
           for fields of more than --host-once-rows rows);
  count / fill / sort   the two list launches and torch.sort of the keys, each
           alone (device events); for the mutex field ``scalar``, its one launch;
  topk     a row_filter_counts_kernel launch over the same field and filter:
           the streaming reference point, it reads the same payload once.

All cases run in one process.  The answers of the two routes are compared for
equality before anything is timed.  Writes <outdir>/extract_rows_bench.json and
<outdir>/README.md.

    python scripts/extract_rows_bench.py --outdir profiles/extract_rows
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

FILTERS = {"1e3": (1, 1_000), "1e5": (2, 100_000), "1e6": (3, 1_000_000)}
FIELDS = {"r64": (64, "set"), "r1000": (1000, "set"), "r50000": (50000, "set"), "mx": (64, "mutex")}


def build_index(base, nshards, threads, fields):
    import numpy as np

    from pilosa_amd import _roaring
    from pilosa_amd.models.field import FieldOptions
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.shardwidth import SHARD_WIDTH
    cols = nshards * SHARD_WIDTH
    h = Holder(base).open()
    idx = h.create_index("c", track_existence=False)
    for name in fields:
        idx.create_field(name, FieldOptions(type="mutex") if FIELDS[name][1] == "mutex"
                         else FieldOptions(cache_type="none"))
    s = idx.create_field("s", FieldOptions(cache_type="none"))
    rng = np.random.default_rng(13)
    for row, n in FILTERS.values():
        c = np.unique(rng.integers(0, cols, n, dtype=np.uint64))
        s.import_bits(np.full(len(c), row, np.uint64), c)
    h.close()
    for name in fields:
        rows, kind = FIELDS[name]
        d = os.path.join(base, "c", name, "views", "standard", "fragments")
        os.makedirs(d, exist_ok=True)
        bpc = 1.0 if kind == "mutex" else min(8.0, rows / 16.0)
        _roaring.write_zipf_fragments(d, 0, nshards, cols, rows, bpc, 1.6, 50.0, 1, threads, cache_size=0)


def stats(ms):
    v = sorted(ms)
    return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(v[len(v) // 10], 4),
            "p90_ms": round(v[(len(v) * 9) // 10], 4), "n": len(v)}


def readme(res):
    """The tables and the default they lead to, from the JSON alone."""
    L = ["# Extract of set-like fields: rows_extract_kernel (K28) against the host function", "",
         f"`scripts/extract_rows_bench.py` on one MI355X (`{res['device']}` by torch's name), one process, "
         f"{res['shards']} shards; medians of "
         f"{res['reps']} runs after {res['warmup']} warm-up runs (p10-p90 in `extract_rows_bench.json`); the host "
         f"request {res['host_reps']} runs (one for fields of more than {res['host_once_rows']:,} rows).  Set fields "
         "of the Zipf generator (s = 1.6, v = 50, seed 1) at min(8, rows / 16) bits per column, a mutex field of 64 "
         "rows at one bit per column on average (the generator does not keep the mutex invariant: a column holds up "
         "to several rows and both routes answer with the smallest; `entries` counts its columns with a row); "
         "filters of about 1e3, 1e5 and 1e6 random columns.  The two routes' answers "
         "were compared for equality in every case before anything was timed.", "",
         "## Request: device against host", "",
         "`device`: `PILOSA_EXTRACT_ROWS_DEVICE=1`; `host`: the same request with `=0`, the host function "
         "(unchanged by this kernel).  Host clock around `Executor.execute`, milliseconds.", "",
         "| field | rows | filter | columns | entries | device | host | host / device |",
         "|---|---|---|---|---|---|---|---|"]
    lost = []
    for c in res["cases"]:
        d, h = c["device_request"]["median_ms"], c["host_request"]["median_ms"]
        L.append(f"| {c['field']} | {c['rows']:,} | {c['filter']} | {c['columns']:,} | {c['entries']:,} | {d:.2f} | "
                 f"{h:.1f} | {h / d:.1f} |")
        if d >= h:
            lost.append(f"{c['field']} / {c['filter']}: device {d:.2f} ms against host {h:.2f} ms ({d / h:.2f} x)")
    L += ["", "## Where the device time goes", "",
          "Device events around each step alone, milliseconds.  `topk`: a `row_filter_counts_kernel` (K25) launch "
          "over the same field and filter, which reads the same payload once and only counts.", "",
          "| field | filter | count | fill | sort | scalar | topk | (count + fill) / topk |",
          "|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        g = lambda k: c[k]["median_ms"] if k in c else None   # noqa: E731
        f = lambda x: "-" if x is None else f"{x:.3f}"        # noqa: E731
        both = (g("count") + g("fill")) if g("fill") is not None else g("scalar")
        L.append(f"| {c['field']} | {c['filter']} | {f(g('count'))} | {f(g('fill'))} | {f(g('sort'))} | "
                 f"{f(g('scalar'))} | {f(g('topk'))} | {both / g('topk'):.2f} |")
    L += ["", "## The default", ""]
    if lost:
        L += ["K28 lost to the host request in:", ""] + [f"* {x}" for x in lost] + \
             ["", "so `EXTRACT_ROWS_DEVICE_DEFAULT` stays `0` (see README \"Known gaps\")."]
    else:
        L += ["K28 beat the host request in every case measured, so `EXTRACT_ROWS_DEVICE_DEFAULT` is `1`: a set, "
              "time, mutex or bool field of Extract() goes to the device unless `PILOSA_EXTRACT_ROWS_DEVICE=0`."]
    L += ["", "Not measured: time fields (the same list modes over the standard view), bool fields (the mutex "
          "path), the headline index (954 shards), filters beyond 2^20 columns (the size guard), "
          "`PILOSA_EXTRACT_ROWS_PER_BLOCK` other than the default 2,048, the 16- and 32-row wave steps, and a "
          "profiler's view of the kernel (occupancy, LDS stalls).", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fields", default="r64,r1000,r50000,mx")
    ap.add_argument("--filters", default="1e3,1e5,1e6")
    ap.add_argument("--shards", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-once-rows", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles", "extract_rows"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from pilosa_amd import shardwidth
    from pilosa_amd.executor import Executor
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.ops.device import Leaf, flat_mask
    from pilosa_amd.ops.gpu_executor import GpuExecutor
    from pilosa_amd.pql import parse_string

    if not torch.cuda.is_available():
        raise SystemExit("extract_rows_bench: no GPU; nothing is measured without one")
    os.environ["PILOSA_EXTRACT_MAX_COLUMNS"] = str(1 << 21)
    os.environ["PILOSA_EXTRACT_DEVICE"] = "1"
    fields = args.fields.split(",")
    base = tempfile.mkdtemp(prefix="pilosa_extract_rows_")
    res = {"bench": "extract_rows", "shards": args.shards, "reps": args.reps, "host_reps": args.host_reps,
           "host_once_rows": args.host_once_rows, "warmup": args.warmup, "cases": []}
    os.makedirs(args.outdir, exist_ok=True)
    try:
        t0 = time.perf_counter()
        build_index(base, args.shards, args.threads, fields)
        shards = list(range(args.shards))
        print(f"index ready ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
        holder = Holder(base).open()
        gpu = GpuExecutor(holder, "cuda:0")
        ex = Executor(holder, gpu=gpu)
        gpu.executor = ex
        eng = gpu.engine
        res["device"] = torch.cuda.get_device_name(0)

        def ev_time(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        def wall(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            return (time.perf_counter() - t) * 1e3

        def median_of(fn, reps, timer=ev_time, warmup=None):
            ms = []
            warmup = args.warmup if warmup is None else warmup
            for i in range(warmup + reps):
                t = timer(fn)
                if i >= warmup:
                    ms.append(t)
            return stats(ms)

        none64 = torch.empty(0, dtype=torch.int64, device=eng.device)
        for name in fields:
            nrows, kind = FIELDS[name]
            view = gpu.view_arena("c", name, "standard", shards)
            view.ensure_keymask()
            S, D = view.S, view.D
            col_base = torch.from_numpy(np.asarray(view.shards, dtype=np.int64) * shardwidth.ARENA_WIDTH).to(eng.device)
            rows_t = eng._rows_tensor(view)
            for fname in args.filters.split(","):
                row, _ = FILTERS[fname]
                filt_text = f"Row(s={row})"
                q = f"Extract({filt_text}, Rows(field={name}))"
                case = {"field": name, "rows": nrows, "D": D, "type": kind, "filter": fname, "query": q}
                box = {}

                def request(key, knob, counted):
                    os.environ["PILOSA_EXTRACT_ROWS_DEVICE"] = knob
                    n0 = gpu.extract_rows_device
                    box[key] = ex.execute("c", q, shards=shards).results[0]
                    assert gpu.extract_rows_device == n0 + counted, f"{key}: the route was not taken"
                host_reps = 1 if nrows > args.host_once_rows else args.host_reps
                # the host runs first; with more than one run the first is a warm-up
                case["host_request"] = median_of(lambda: request("host", "0", 0), host_reps, wall,
                                                 warmup=1 if host_reps > 1 else 0)
                case["device_request"] = median_of(lambda: request("dev", "1", 1), args.reps, wall)
                assert box["dev"] == box["host"], "device and host answers differ"
                os.environ["PILOSA_EXTRACT_ROWS_DEVICE"] = "1"
                case["columns"] = keep = len(box["dev"])

                # ---- the steps alone: offsets as GpuEngine.bsi_extract computes them
                filt = gpu.plan("c", parse_string(filt_text).calls[0], shards)
                assert type(filt) is Leaf
                progs, ordered = eng._bsi_filter_program([filt], view)
                tp, tv = eng.upload_batch(progs, ordered)
                counts = torch.zeros(S * 16, dtype=torch.int32, device=eng.device)
                eng.ext.expr_count(tp, tv, S, none64, counts, 2 if bool(flat_mask(progs).all()) else 0)
                c64 = counts.to(torch.int64)
                ends = torch.cumsum(c64, 0)
                unit_off = torch.where(c64 > 0, ends - c64, torch.full_like(ends, -1)).contiguous()
                assert int(ends[-1]) == keep
                rpb = eng.EXTRACT_ROWS_PER_BLOCK

                def launch(mode, wg, keys, first):
                    eng.ext.rows_extract(mode, tp, tv, S, 0, D, rpb, 0, unit_off, col_base, keep, none64, wg, keys,
                                         rows_t if mode == 3 else none64, first)
                if kind == "mutex":
                    first = torch.full((keep,), -1, dtype=torch.int64, device=eng.device)
                    case["scalar"] = median_of(lambda: launch(3, none64, none64, first), args.reps)
                    case["entries"] = int((first != -1).sum())
                else:
                    blocks = int(eng.ext.rows_extract_blocks(S, D, rpb))
                    wg = torch.zeros(blocks, dtype=torch.int64, device=eng.device)
                    case["count"] = median_of(lambda: launch(1, wg, none64, none64), args.reps)
                    wg_end = torch.cumsum(wg, 0)
                    case["entries"] = T = int(wg_end[-1])
                    case["workgroups"] = blocks
                    assert T == len(box["dev"].data[0][1])
                    wg_base = (wg_end - wg).contiguous()
                    keys = torch.full((T,), -1, dtype=torch.int64, device=eng.device)
                    case["fill"] = median_of(lambda: launch(2, wg_base, keys, none64), args.reps)
                    case["sort"] = median_of(lambda: torch.sort(keys), args.reps)
                case["topk"] = median_of(lambda: eng.row_filter_counts(view, filt), args.reps)
                res["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
                with open(os.path.join(args.outdir, "extract_rows_bench.json"), "w") as fh:
                    fh.write(json.dumps(res) + "\n")     # kept current: a later case may run long
            del view
            torch.cuda.empty_cache()
        ex.close()
        holder.close()
    finally:
        shutil.rmtree(base, ignore_errors=True)
    with open(os.path.join(args.outdir, "README.md"), "w") as fh:
        fh.write(readme(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
