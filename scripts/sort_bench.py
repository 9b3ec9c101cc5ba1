#!/usr/bin/env python3
"""Sort(<filter>, field=, limit=, sort-desc=): what a call costs on the device
and on the host.

The index is the profiles/extract shape: --shards shards (64), one depth-20
int field ``v`` whose planes are bitmap containers, half the columns holding a
value.  The filters are none (case ``all``) and two rows of a set field ``s``
with about 1e5 and 1e6 random columns over all shards (cases ``1e5``,
``1e6``); about half of a filter's columns hold a value and are considered.

Reported per case, limit (--limits) and direction, each a median over --reps
runs with p10 / p90 / min / max:

  device    the request through Executor.execute on the device route (the
            descent, the two bsi_sort_select_kernel launches, the device sort
            and the one copy of the answer);
  host      the same request with PILOSA_SORT_DEVICE=0 (--host-reps runs; one
            run for the unfiltered case);
  recipe    where the filter fits Extract's size guard: what a client did
            before Sort() existed -- Extract(filter, Rows(field=v)) on the
            device route plus a numpy lexsort of the answer;

and per case and direction, at every limit:

  count / fill   bsi_sort_select_kernel alone, mode 1 and mode 2 (device events
            around the launch; the descent and the cumsums are done once,
            outside), for every n in --slots at the first limit, then at the
            request's n;
  sum       the bsi_sum launch over the same field and filter, the reference
            point: that kernel reads the same planes exactly once.

    python scripts/sort_bench.py --out sort_bench.json
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
CASES = {"all": (0, None), "1e5": (2, 100_000), "1e6": (3, 1_000_000)}


def build_index(base, nshards, threads):
    import numpy as np

    from pilosa_amd import _roaring
    from pilosa_amd.models.field import FieldOptions
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.shardwidth import SHARD_WIDTH
    cols = nshards * SHARD_WIDTH
    h = Holder(base).open()
    idx = h.create_index("c", track_existence=False)
    f = idx.create_field("v", FieldOptions(type="int", min=-1000, max=1_000_000))
    f.options.bit_depth = DEPTH
    f.bsi.bit_depth = DEPTH
    f.save_meta()
    s = idx.create_field("s", FieldOptions(cache_type="none"))
    rng = np.random.default_rng(13)
    for row, n in CASES.values():
        if n:
            c = np.unique(rng.integers(0, cols, n, dtype=np.uint64))
            s.import_bits(np.full(len(c), row, np.uint64), c)
    h.close()
    d = os.path.join(base, "c", "v", "views", "bsig_v", "fragments")
    os.makedirs(d, exist_ok=True)
    _roaring.write_bsi_fragments(d, 0, nshards, cols, DEPTH, 0.5, -1000, 1_000_000, 7, threads)


def stats(ms):
    v = sorted(ms)
    return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(v[len(v) // 10], 4),
            "p90_ms": round(v[(len(v) * 9) // 10], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="all,1e5,1e6")
    ap.add_argument("--limits", default="10,1000,100000")
    ap.add_argument("--shards", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slots", default="1,2,4,8")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from pilosa_amd import shardwidth
    from pilosa_amd.executor import Executor, SortedColumns, _extract_max_columns
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.ops.gpu_executor import EMPTY, GpuExecutor, sort_slots_env
    from pilosa_amd.pql import parse_string

    base = tempfile.mkdtemp(prefix="pilosa_sort_")
    limits = [int(x) for x in args.limits.split(",")]
    res = {"bench": "sort", "shards": args.shards, "depth": DEPTH, "reps": args.reps, "host_reps": args.host_reps,
           "limits": limits, "cases": {}}
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
        req_slots = int(eng.ext.sort_slots(DEPTH, sort_slots_env()))
        res["request_slots"] = req_slots

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
        S = bv.S
        col_base = torch.from_numpy(np.asarray(bv.shards, dtype=np.int64) * shardwidth.ARENA_WIDTH).to(eng.device)
        e64 = torch.empty(0, dtype=torch.int64, device=eng.device)
        for case in args.cases.split(","):
            row, _ = CASES[case]
            filt_text = f"Row(s={row})" if row else ""
            out = {"filter": filt_text, "rows": []}
            filt = gpu.plan("c", parse_string(filt_text).calls[0], shards) if row else None
            assert filt is not EMPTY
            out["sum"] = median_of(lambda: eng.bsi_sum_async([filt], bv, DEPTH, matrix=False), args.reps)
            recipe_ok = None
            for desc in (False, True):
                for li, lim in enumerate(limits):
                    r = {"limit": lim, "desc": desc}
                    # ---- the two launches alone, behind one descent
                    n_con, T, _, (tp, tv, targs) = eng.bsi_kth(
                        filt, bv, DEPTH, rank=lambda n: None if lim >= n else (n - lim + 1 if desc else lim))
                    out["considered"] = n_con
                    k = min(lim, n_con)
                    r["kernel"] = []
                    for n in ([int(x) for x in args.slots.split(",")] if li == 0 else [req_slots]):
                        used = int(eng.ext.sort_slots(DEPTH, n))
                        if used != n:
                            r["kernel"].append({"slots": n, "clamped_to": used})
                            continue
                        blocks = int(eng.ext.sort_blocks(S, n))
                        counts = torch.zeros(blocks * 2, dtype=torch.int32, device=eng.device)

                        def count():
                            eng.ext.bsi_sort_select(1, tp, tv, S, targs, n, T is None, desc, int(T or 0), counts, e64,
                                                    e64, e64, e64, 0, e64, e64)
                        kr = {"slots": n, "count": median_of(count, args.reps)}
                        c64 = counts.view(blocks, 2).to(torch.int64)
                        ends = torch.cumsum(c64, 0)
                        offs = ends - c64
                        m = (k - ends[-1, 0]).clamp(min=0).reshape(1).contiguous()
                        bo, eb = offs[:, 0].contiguous(), offs[:, 1].contiguous()
                        columns = torch.full((k,), -1, dtype=torch.int64, device=eng.device)
                        values = torch.zeros(k, dtype=torch.int64, device=eng.device)

                        def fill():
                            eng.ext.bsi_sort_select(2, tp, tv, S, targs, n, T is None, desc, int(T or 0), counts, bo,
                                                    eb, m, col_base, -1000, columns, values)
                        kr["fill"] = median_of(fill, args.reps)
                        assert int((columns >= 0).sum()) == k, "the fill pass left slots unreached"
                        r["kernel"].append(kr)
                    # ---- request level: device route, then the host path on the same index
                    q = "Sort(" + (filt_text + ", " if row else "") + f"field=v, limit={lim}" + \
                        (", sort-desc=true" if desc else "") + ")"
                    r["query"] = q
                    os.environ["PILOSA_SORT_DEVICE"] = "1"
                    box = {}

                    def dev():
                        n0 = gpu.sort_device
                        box["dev"] = ex.execute("c", q, shards=shards).results[0]
                        assert gpu.sort_device == n0 + 1, "the device route declined"
                    r["device_request"] = median_of(dev, args.reps, lambda fn: timed(fn)[0])
                    os.environ["PILOSA_SORT_DEVICE"] = "0"

                    def host():
                        n0 = gpu.sort_device
                        box["host"] = ex.execute("c", q, shards=shards).results[0]
                        assert gpu.sort_device == n0
                    r["host_request"] = stats([timed(host)[0] for _ in range(args.host_reps if row else 1)])
                    os.environ["PILOSA_SORT_DEVICE"] = "1"
                    assert box["dev"] == box["host"] and len(box["dev"]) == k, "device and host answers differ"
                    # ---- the client recipe of before: Extract everything, sort on the client
                    if row and recipe_ok is not False:
                        eq = f"Extract({filt_text}, Rows(field=v))"

                        def recipe():
                            t = ex.execute("c", eq, shards=shards).results[0]
                            vals, ok = t.data[0]
                            cols, vals = t.columns[ok], vals[ok]
                            order = np.lexsort((cols, ~vals if desc else vals))[:lim]
                            box["recipe"] = SortedColumns(cols[order], vals[order])
                        try:
                            r["recipe_request"] = median_of(recipe, max(3, args.reps // 4), lambda fn: timed(fn)[0])
                            assert box["recipe"] == box["dev"], "the recipe and the device answers differ"
                            recipe_ok = True
                        except Exception as err:   # the size guard: the recipe does not exist for this filter
                            if recipe_ok or "exceed the limit" not in str(err):
                                raise
                            recipe_ok = False
                            out["recipe"] = f"refused: {err} (cap {_extract_max_columns()})"
                    out["rows"].append(r)
                    print(json.dumps({case: r}), file=sys.stderr, flush=True)
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
