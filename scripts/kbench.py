#!/usr/bin/env python3
"""Kernel-level A/B harness on the headline dataset: times the device half
(launch_count) of a Count(Intersect) batch for several engine settings with
HIP events.  Usage: python scripts/kbench.py [--batch 1024] [--reps 5] [--shards N]

Pair-kernel variants (--variants): 6 = the plain v6 kernel (39, batched
staging, for batches of up to 128 queries when the chunk size is 0), 63 = the
bitmap twins (64 queries per wave); --twin-cutoff lists the cutoffs T variant
63 is timed at (the twin is rebuilt per T).  A variant may be listed several
times to alternate it with others.  --hot-rows times the kernels with the
hot-pair table of H rows (DeviceView.ensure_hot) next to H = 0 on the same
arena, and prints how many entries it answers.  --compact 0,1 alternates
today's route and the one that compacts the table-answered queries out of the
pair grid (GpuEngine.use_compact) for every such setting, in one process on one
arena; --row-mod 512 draws every row from the table's rows (a batch with no
live query: the compacted route's oversized-grid tail).  The pair kernels are
the same in both modules; PILOSA_HIPKERNELS=_hipkernels runs the shipped one."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the A/B module: the shipped kernels plus the TopN cost-isolation bits
# (python -m pilosa_amd.native.build --kbench)
os.environ.setdefault("PILOSA_HIPKERNELS", "_hipkernels_kbench")
sys.path.insert(0, ROOT)

from bench import NROWS, SHARD_WIDTH, TOTAL_COLS, zipf_rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shards", type=int, default=0, help="0 = full 954")
    ap.add_argument("--cq", default="0,32,64", help="pair-kernel chunk sizes (queries per wave)")
    ap.add_argument("--no-tile", action="store_true", help="skip the generic tile kernel")
    ap.add_argument("--variants", default="", help="pair-kernel variants at --cq's first size, e.g. 6,63 (39@8: at 8 queries per wave)")
    ap.add_argument("--twin-cutoff", default="", help="twin cutoffs T for variant 63, e.g. 3072,2730,2048 "
                    "(default: DeviceView.TWIN_CUTOFF)")
    ap.add_argument("--hot-rows", default="", help="hot-pair table sizes H each --variants setting of the shipped "
                    "kernels (6, 39, 63) is timed at, e.g. 0,128,256,512 (0 = no table; default: no table)")
    ap.add_argument("--compact", default="", help="0,1: time each --variants setting on today's route (0) and "
                    "with the table-answered queries compacted out of the pair grid (1); default: the engine's own")
    ap.add_argument("--row-mod", type=int, default=0, help="take the batch's row ids modulo this (0 = as drawn)")
    args = ap.parse_args()
    import torch

    from pilosa_amd import _roaring
    from pilosa_amd.ops.device import DeviceView, GpuEngine
    from pilosa_amd.ops.planner import NativeCountCompiler

    dev = torch.device("cuda", 0)
    nshards = args.shards or math.ceil(TOTAL_COLS / SHARD_WIDTH)
    arena = _roaring.gen_zipf_arena(0, nshards, TOTAL_COLS, NROWS, 8.0, 1.6, 50.0, 1, 16)
    view = DeviceView(*arena, dev, shards=list(range(nshards)))
    del arena
    rng = np.random.default_rng(1234)
    ra, rb = zipf_rows(rng, args.batch), zipf_rows(rng, args.batch)
    if args.row_mod:
        ra, rb = ra % args.row_mod, rb % args.row_mod
    qs = [f"Count(Intersect(Row(f={a}), Row(f={b})))" for a, b in zip(ra, rb)]
    progs, views, S = NativeCountCompiler({"f": view}).compile(qs)
    results = {}
    ref = None
    configs = [] if args.no_tile else [("tile", {"use_and2": False})]
    configs += [(f"and2_cq{c}", {"and2_cq": int(c), "and2_variant": 1}) for c in args.cq.split(",") if c]
    cq0 = int(args.cq.split(",")[0]) if args.cq else 64
    for v in args.variants.split(","):
        if not v:
            continue
        vv, _, cq = v.partition("@")   # "39@8": variant 39 at 8 queries per wave
        cq = int(cq) if cq else cq0
        cuts = [int(t) for t in args.twin_cutoff.split(",") if t] if int(vv) == 63 else []
        hots = [int(h) for h in args.hot_rows.split(",") if h] if int(vv) in (6, 39, 63) else []
        compacts = [int(c) for c in args.compact.split(",") if c]
        for t in cuts or [None]:
            for hr in hots or [0]:
                for cp in compacts or [None]:
                    name = f"and2var{vv}_cq{cq}" + (f"_t{t}" if t is not None else "") + (f"_h{hr}" if hr else "") + \
                        (f"_c{cp}" if cp is not None else "")
                    while name in [c[0] for c in configs]:
                        name += "'"      # a repeat of the same setting (alternating runs)
                    configs.append((name, {"and2_cq": cq, "and2_variant": int(vv), "twin_cutoff": t, "hot_rows": hr,
                                           "compact": cp}))
    for name, cfg in configs:
        eng = GpuEngine(dev)
        cut = cfg.pop("twin_cutoff", None)
        hot = cfg.pop("hot_rows", 0)
        compact = cfg.pop("compact", None)
        for k, v in cfg.items():
            setattr(eng, k, v)
        eng.use_twin = cfg.get("and2_variant") == 63   # variants are explicit here: 6 is the plain kernel
        if cut is not None and (view.TWIN_CUTOFF != cut or not view.twin_fresh()):
            view._twin = None        # rebuilt at this cutoff by prepare_progs
            view.TWIN_CUTOFF = cut
        eng.use_hot = hot > 0        # the table is explicit too
        if compact is not None:      # and so is the route: any batch above the serving sizes
            eng.use_compact = bool(compact)
            eng.PAIR_COMPACT_MIN = 1
        if hot and (view.HOTPAIR_ROWS != hot or getattr(view, "_hot", None) is None):
            view._hot = None         # rebuilt at this size by prepare_progs
            view.HOTPAIR_ROWS = hot
            view.HOTPAIR_MIN_CONTAINERS = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            view.ensure_hot()
            hp = view._hot
            if hp is not None:
                print(f"hot-pair table H={hp.h}: {hp.counts.numel() * 4 / 2**20:.0f} MiB, "
                      f"build {time.perf_counter() - t0:.3f} s", flush=True)
        t0 = time.perf_counter()
        h = eng.prepare_progs(progs, views, S)
        if hot:
            # how much of the batch the table answers: marked entries of the pairs buffer
            (tp, _, _, n), = h[3]
            pr = torch.empty(S * 16 * n * 2, dtype=torch.int32, device=dev)
            pt = torch.empty(S * 16 * n, dtype=torch.int32, device=dev)
            eng.ext.and2_count(tp, h[2], S, pr, pt, eng.and2_cq, cfg["and2_variant"])
            marked = int((pr.view(-1, 2)[:, 0] == -2).sum().item())
            print(f"{name}: {marked} of {S * n} (shard, query) entries precounted ({marked / (S * n):.1%})", flush=True)
            del pr, pt
        if cut is not None and view.twin_fresh():
            tw = view._twin
            print(f"twin T={cut}: {len(tw[4])} rows, {tw[1].numel() * 8 / 2**30:.2f} GiB, "
                  f"prepare+build {time.perf_counter() - t0:.3f} s", flush=True)
        out = eng.launch_count(h)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        if ref is None:
            ref = got
        ok = bool(np.array_equal(got, ref)) or name.startswith("dbg")
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.launch_count(h)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        results[name] = {"ms_min": round(min(ts), 3), "ms_med": round(sorted(ts)[len(ts) // 2], 3), "match": ok}
        print(name, results[name], flush=True)
    print(json.dumps({"batch": args.batch, "shards": nshards, "results": results}))


if __name__ == "__main__":
    main()
