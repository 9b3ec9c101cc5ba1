#!/usr/bin/env python3
"""Kernel-level timing of TopK's two device routes on a 64-shard Zipf view:
row_filter_counts_kernel (one pass, the filter staged once per (shard, key))
against the per-row programs route (one filter & row program per row through
count_per_shard_progs), at several row counts and three filter shapes (none, a
sparse row, a dense expression).  Per cell: warm-up, then the median of
device-event timings of the device work alone (programs compiled beforehand),
and the median wall time of the whole route from expressions to the count
vector on the device.  The two count vectors are compared before anything is
timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=64)
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1000, 10000, 50000])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["0:64", "2048:64", "2048:0"],
                    help="row_filter_counts_kernel launch shapes to time, <rows per workgroup>:<rows per wave "
                         "step> (0 rows per workgroup = one workgroup per (shard, key); 0 rows per wave = the "
                         "default choice)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import SHARD_WIDTH
    from pilosa_amd import _roaring
    from pilosa_amd.ops.device import DeviceView, GpuEngine, Leaf, Op
    from pilosa_amd.ops.gpu_executor import MAX_GROUPS_PER_LAUNCH

    dev = torch.device("cuda", 0)
    S = args.shards
    cols = S * SHARD_WIDTH
    eng = GpuEngine(dev)
    # the filter field: 1,000 Zipf rows, one bit per column (bench.py's filter field)
    fv = DeviceView(*_roaring.gen_zipf_arena(0, S, cols, 1000, 1.0, 1.6, 50.0, 11, 16), dev, shards=list(range(S)))
    filters = {"none": None, "sparse row": Leaf(fv, 900),
               "dense expr": Op("or", (Leaf(fv, 0), Op("or", (Leaf(fv, 1), Leaf(fv, 2)))))}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1000)
            ev.append(e0.elapsed_time(e1))
        return round(statistics.median(ev), 3), round(statistics.median(wall), 3)

    out = {"shards": S, "reps": args.reps, "warmup": args.warmup, "cells": []}
    for R in args.rows:
        bpc = min(8.0, R / 16.0)
        view = DeviceView(*_roaring.gen_zipf_arena(0, S, cols, R, bpc, 1.6, 50.0, 1, 16), dev, shards=list(range(S)))
        view.ensure_keymask()
        meta = view.t_meta.cpu().numpy()
        types = np.bincount((meta >> 4) & 3, minlength=4).tolist()
        for fname, filt in filters.items():
            def kernel_route():
                f = filt
                if f is not None and type(f) is not Leaf:
                    f = Leaf(eng.dense_view(f), 0)
                return eng.row_filter_counts(view, f)

            rows = [int(r) for r in view.rows]
            chunks = [rows[i:i + MAX_GROUPS_PER_LAUNCH] for i in range(0, len(rows), MAX_GROUPS_PER_LAUNCH)]

            def exprs_of(part):
                return [Leaf(view, r) if filt is None else Op("and", (filt, Leaf(view, r))) for r in part]
            compiled = [eng.compile_batch(exprs_of(p)) for p in chunks]

            def programs_device():
                return torch.cat([eng.count_per_shard_progs(p, v, s, as_tensor=True).sum(dim=1)
                                  for p, v, s in compiled])

            def programs_route():
                return torch.cat([eng.count_per_shard_progs(*eng.compile_batch(exprs_of(p)), as_tensor=True).sum(dim=1)
                                  for p in chunks])
            dense = view.dense_many(np.asarray(rows, np.uint64))
            want = programs_device().cpu().numpy()
            cell = {"rows": R, "D": view.D, "containers": int(view.container_count),
                    "types[_, array, bitmap, run]": types, "filter": fname, "nonzero_rows": int((want > 0).sum())}
            for shape in args.shapes:
                rpb, rpw = shape.split(":")
                os.environ["PILOSA_TOPK_ROWS_PER_BLOCK"] = rpb
                os.environ["PILOSA_TOPK_ROWS_PER_WAVE"] = rpw
                got = kernel_route().cpu().numpy()[dense]
                assert (got == want).all(), (R, fname, shape)
                cell[f"kernel_{shape}_ms[device, wall]"] = timed(kernel_route)
            os.environ.pop("PILOSA_TOPK_ROWS_PER_BLOCK", None)
            os.environ.pop("PILOSA_TOPK_ROWS_PER_WAVE", None)
            cell["programs_ms[device, wall]"] = timed(programs_device)
            cell["programs_with_compile_wall_ms"] = timed(programs_route)[1]
            out["cells"].append(cell)
            print(json.dumps(cell), flush=True)
        del view
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh)


if __name__ == "__main__":
    main()
