#!/usr/bin/env python3
"""GroupBy(..., aggregate=Sum(field=v)): what a request costs

  (dev_group_sum)  through Executor.execute with bsi_group_sum_kernel;
  (dev_per_filter) the same request with the group programs sent through the
           per-filter kernel (bsi_sum_keys_kernel) instead;
  (host)   the same call on the host path (PILOSA_GROUPSUM_DEVICE=0);
  (client) what a client had to do before the argument existed: the plain
           GroupBy, then one Sum(Intersect(Row(a=..), Row(b=..)), field=v) per
           returned group in as few requests as the batch's memory allows
           (bsi_sum_batch);

and, at kernel level, bsi_group_sum at several slab sizes against the
per-filter kernel (bsi_sum_async with the matrix path off) fed the same group
programs, timed with device events.  --kernels-only runs just that part, for a
kernel trace of its own.

The index: --shards shards, int field v (depth 20, half the columns hold a
value), set fields a and b of 32 rows each with Zipf row densities, all
generated from fixed seeds.  Three shapes: Rows(a) x Rows(b) (about 1,024
groups), Rows(a) (32) and Rows(a, limit=8) (8).  Every variant is warmed, the
variants of one comparison alternate request by request, and their answers are
compared for equality.

    python scripts/groupby_sum_bench.py --reps 30 --out result.json
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
SHAPES = (("1024", "Rows(a), Rows(b)", ("a", "b")), ("32", "Rows(a)", ("a",)), ("8", "Rows(a, limit=8)", ("a",)))


def build_index(base, nshards, threads):
    from pilosa_amd import _roaring
    from pilosa_amd.models.field import FieldOptions
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.shardwidth import SHARD_WIDTH
    cols = nshards * SHARD_WIDTH
    h = Holder(base).open()
    idx = h.create_index("c", track_existence=False)
    fv = idx.create_field("v", FieldOptions(type="int", min=-1000, max=1_000_000))
    fv.options.bit_depth = DEPTH
    fv.bsi.bit_depth = DEPTH
    fv.save_meta()
    for name in ("a", "b"):
        idx.create_field(name, FieldOptions(cache_type="none"))
    h.close()

    def frag_dir(field, view):
        d = os.path.join(base, "c", field, "views", view, "fragments")
        os.makedirs(d, exist_ok=True)
        return d
    _roaring.write_bsi_fragments(frag_dir("v", "bsig_v"), 0, nshards, cols, DEPTH, 0.5, -1000, 1_000_000, 7, threads)
    for name, seed in (("a", 11), ("b", 12)):
        _roaring.write_zipf_fragments(frag_dir(name, "standard"), 0, nshards, cols, 32, 1.0, 1.6, 50.0, seed, threads,
                                      cache_size=0)


def stats(ms):
    v = sorted(ms)
    return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(v[len(v) // 10], 4),
            "p90_ms": round(v[(len(v) * 9) // 10], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
            "n": len(v)}


def flat(groups):
    return [(g.key(), g.count, g.sum, g.sum_count) for g in groups]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shards", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30, help="timed requests per variant")
    ap.add_argument("--host-reps", type=int, default=None, help="timed host-path requests (default: --reps)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slabs", default="3,5,7,10,13")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--part-bytes", type=int, default=16 << 30, help="dense filter rows one client request may hold")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    host_reps = args.reps if args.host_reps is None else args.host_reps

    import torch

    from pilosa_amd.executor import Executor
    from pilosa_amd.models.holder import Holder
    from pilosa_amd.ops.device import Leaf, Op
    from pilosa_amd.ops.gpu_executor import GpuExecutor

    base = tempfile.mkdtemp(prefix="pilosa_gbs_")
    res = {"bench": "groupby_sum", "shards": args.shards, "depth": DEPTH, "reps": args.reps, "host_reps": host_reps}
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

        def one(q):
            return ex.execute("c", q, shards=shards).results[0]

        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            return (time.perf_counter() - t) * 1e3, r

        res["requests"], res["kernels"] = [], []
        for name, children, fields in SHAPES:
            agg_q = f"GroupBy({children}, aggregate=Sum(field=v))"
            groups = one(f"GroupBy({children})")
            G, S = len(groups), args.shards
            keys = [g.key() for g in groups]
            arenas = [gpu.view_arena("c", f, "standard", shards) for f in fields]
            bv = gpu.view_arena("c", "v", "bsig_v", shards)
            # ---- kernel level: same G programs, device events around each call
            progs, views = gpu._key_programs(arenas, keys, None)
            exprs = [Op("and", tuple(Leaf(arenas[x], key[x]) for x in range(len(key)))) if len(key) > 1
                     else Leaf(arenas[0], key[0]) for key in keys]

            def ev_time(fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = fn()
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b), [t.cpu().tolist() for t in out]
            slabs = [int(x) for x in args.slabs.split(",")]
            kvars = [("per_filter", lambda: eng.bsi_sum_async(exprs, bv, DEPTH, matrix=False))]
            for p in slabs:
                def run(p=p):
                    os.environ["PILOSA_GROUPSUM_SLAB"] = str(p)
                    try:
                        return eng.bsi_group_sum(progs, views, bv, DEPTH)
                    finally:
                        del os.environ["PILOSA_GROUPSUM_SLAB"]
                kvars.append((f"group_sum_P{p}", run))
            kms = {n: [] for n, _ in kvars}
            ref = None
            for rep in range(args.warmup + args.reps):
                for n, fn in kvars:
                    ms, out = ev_time(fn)
                    ref = out if ref is None else ref
                    assert out == ref, f"{n} disagrees with the per-filter kernel"
                    if rep >= args.warmup:
                        kms[n].append(ms)
            nslab = {p: -(-DEPTH // p) for p in slabs}
            chunks = -(-G // eng.GROUPSUM_CHUNK)
            krow = {"groups": G, "tile_loads_per_shard_key": {
                "per_filter": G * (DEPTH + 2),
                **{f"group_sum_P{p}": (DEPTH + 2 * nslab[p]) * chunks for p in slabs}},
                "group_container_loads_per_shard_key": {f"group_sum_P{p}": G * len(fields) * nslab[p] for p in slabs},
                **{n: stats(v) for n, v in kms.items()}}
            res["kernels"].append(krow)
            print(json.dumps(krow), file=sys.stderr, flush=True)
            if args.kernels_only:
                continue

            # ---- request level
            def run_kernel():
                os.environ["PILOSA_GROUPSUM_MIN_GROUPS"] = "1"
                try:
                    n0 = gpu.group_sum_device
                    r = flat(one(agg_q))
                finally:
                    del os.environ["PILOSA_GROUPSUM_MIN_GROUPS"]
                assert gpu.group_sum_device == n0 + 1, "bsi_group_sum_kernel did not answer"
                return r

            def run_per_filter():
                os.environ["PILOSA_GROUPSUM_MIN_GROUPS"] = str(1 << 40)
                try:
                    n0 = gpu.group_sum_per_filter
                    r = flat(one(agg_q))
                finally:
                    del os.environ["PILOSA_GROUPSUM_MIN_GROUPS"]
                assert gpu.group_sum_per_filter == n0 + 1, "the per-filter kernel did not answer"
                return r

            def run_host():
                os.environ["PILOSA_GROUPSUM_DEVICE"] = "0"
                try:
                    return flat(one(agg_q))
                finally:
                    del os.environ["PILOSA_GROUPSUM_DEVICE"]
            parts = max(1, -(-G * S * (128 << 10) // args.part_bytes))
            per = -(-G // parts)

            def run_client():
                gs = one(f"GroupBy({children})")
                out = []
                for i in range(0, len(gs), per):
                    q = " ".join("Sum(" + (f"Intersect({', '.join(f'Row({fr.field}={fr.row_id})' for fr in g.group)})"
                                           if len(g.group) > 1 else
                                           f"Row({g.group[0].field}={g.group[0].row_id})") + ", field=v)"
                                 for g in gs[i:i + per])
                    out += ex.execute("c", q, shards=shards).results
                return [(g.key(), g.count, vc.val, vc.count) for g, vc in zip(gs, out)]
            # --host-reps applies to the large shape only (a host request there takes seconds)
            variants = [("dev_group_sum", run_kernel, args.reps), ("dev_per_filter", run_per_filter, args.reps),
                        ("client", run_client, args.reps),
                        ("host", run_host, host_reps if G > 64 else args.reps)]
            answers = {}
            for n, fn, reps in variants:
                for _ in range(args.warmup if reps else 0):
                    answers[n] = fn()
            assert all(a == answers["dev_group_sum"] for a in answers.values()), "variants disagree"
            ms = {n: [] for n, _, _ in variants}
            for rep in range(max(r for _, _, r in variants)):
                for n, fn, reps in variants:      # alternating, request by request
                    if rep < reps:
                        t, out = timed(fn)
                        assert out == answers["dev_group_sum"], f"{n} changed its answer"
                        ms[n].append(t)
            row = {"groups": G, "client_parts": parts, **{n: stats(v) for n, v in ms.items() if v}}
            res["requests"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
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
