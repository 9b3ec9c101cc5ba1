#!/usr/bin/env python3
"""Work profile of the pair kernel on the headline batch (host-side, same
arena / batch as scripts/kbench.py): per (unit, 64-query chunk) the v6 walk
-- pairs, stagings of A (a new leaf-0 container), A and B types and sizes,
run lengths -- so kernel restructures can be priced before they are built.
Also: LDS probes (one per array B value) per B size class, array stagings per
A size class, and the pairs / probes / stagings whose A or B container a
bitmap twin at cutoff T would replace (rows picked by select_twin_rows over
the sampled shards, containers by n > T) with the bytes that adds.
Hot-pair table (--hot-rows H,...): with the H rows of most bits answered
from the per-shard count table whenever both rows of a query are among them,
what remains in the pair kernel as a share of today -- queries answered,
pairs, array probes, bitmap / twin B pairs, stagings, referenced bytes (twins
at --hot-twin-cutoff, the planner's dedupe ignored).
Compaction ("compaction", per H, repeated queries removed as the planner
does): the columns of a (shard, key) unit's pairs / partial rows and its
64-query waves today and with the table-answered queries taken out of the
grid, the live lanes per wave, and the run lengths of equal leaf 0 among the
live queries (a run of one is a staging no other query shares).
Usage: python scripts/pair_stats.py [--sample 2] [--batch 4096] [--twin-cutoff 3072,2730,2048]
       [--hot-rows 64,128,256,512,1024] [--seed 1234]"""
import argparse
import collections
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import NROWS, TOTAL_COLS, zipf_rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cq", type=int, default=64)
    ap.add_argument("--twin-cutoff", default="3072,2730,2048")
    ap.add_argument("--hot-rows", default="64,128,256,512,1024")
    ap.add_argument("--hot-twin-cutoff", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    from pilosa_amd import _roaring
    from pilosa_amd.ops.device import select_twin_rows
    rows, rowptr, sb, meta, payload = _roaring.gen_zipf_arena(0, args.sample, TOTAL_COLS, NROWS, 8.0, 1.6, 50.0, 1, 8)
    rows = np.asarray(rows, np.uint64)
    D = len(rows)
    rp = np.asarray(rowptr).reshape(args.sample, D + 1).astype(np.int64)
    sb = np.asarray(sb, np.int64)
    meta = np.asarray(meta, np.int64)
    typ = (meta >> 4) & 3
    n = (meta >> 6) & 0x1FFFF
    jj = meta & 15
    rng = np.random.default_rng(args.seed)
    ra, rb = zipf_rows(rng, args.batch), zipf_rows(rng, args.batch)
    keys = np.concatenate([ra, rb])
    u, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    ca, cbb = cnt[inv[:len(ra)]], cnt[inv[len(ra):]]
    sw = (cbb > ca) | ((cbb == ca) & (rb < ra))
    A = np.where(sw, rb, ra)
    B = np.where(sw, ra, rb)
    o = np.lexsort((B, A))
    A, B = A[o], B[o]
    dense = {int(r): i for i, r in enumerate(rows.tolist())}
    st = collections.Counter()
    nb_hist = collections.Counter()
    na_stage_hist = collections.Counter()
    runlen = collections.Counter()
    pairs_per_wave = []
    cuts = [int(t) for t in args.twin_cutoff.split(",") if t]
    sample = [(rp[s], meta[sb[s]:sb[s] + rp[s, -1]]) for s in range(args.sample)]
    twin_rows = {t: set(select_twin_rows(sample, D, t, 64).tolist()) for t in cuts}
    probes = collections.Counter()        # array B values probed, per B size class
    stage_cls = collections.Counter()     # array A stagings per size class
    tw = {t: collections.Counter() for t in cuts}
    ref_bytes = 0                         # bytes the kernel references (A per staging, B per pair)
    # hot-pair table: the H dense rows with the most bits over the sample
    hots = [int(h) for h in args.hot_rows.split(",") if h]
    bits = np.zeros(D, np.int64)
    for s in range(args.sample):
        bits += np.bincount(np.repeat(np.arange(D), np.diff(rp[s])), weights=n[sb[s]:sb[s] + rp[s, -1]],
                            minlength=D).astype(np.int64)
    by_bits = np.argsort(-bits, kind="stable")
    hot_set = {h: set(by_bits[:h].tolist()) for h in hots}
    hot_twin = set(select_twin_rows(sample, D, args.hot_twin_cutoff, 64).tolist())
    hot = {h: collections.Counter() for h in [0] + hots}   # 0 = today
    dA = np.array([dense.get(int(r), -1) for r in A])
    dB = np.array([dense.get(int(r), -1) for r in B])
    for h in hots:
        hot[h]["queries_answered"] = int(sum(1 for a, b in zip(dA, dB) if a in hot_set[h] and b in hot_set[h]))

    # compaction: query-level, the same for every (shard, key) unit
    uq = np.unique(np.stack([dA, dB], axis=1), axis=0)     # sorted by (A, B), duplicates removed
    compaction = {}
    for h in hots:
        hs = np.fromiter(hot_set[h], np.int64)
        live = ~(np.isin(uq[:, 0], hs) & np.isin(uq[:, 1], hs))
        waves = [live[c0:c0 + args.cq] for c0 in range(0, len(uq), args.cq)]
        la = uq[live, 0]
        starts = np.flatnonzero(np.concatenate([[True], la[1:] != la[:-1]])) if len(la) else np.zeros(0, np.int64)
        lens = np.diff(np.concatenate([starts, [len(la)]]))
        nl = int(live.sum())
        wc = -(-nl // args.cq)
        hist = collections.Counter(int(min(x, 64)) for x in lens)
        compaction[str(h)] = {
            "queries_in_grid": {"today": len(uq), "compacted": nl},
            "waves_per_unit": {"today": len(waves), "entirely_table_answered": int(sum(1 for w in waves if not w.any())),
                               "compacted": wc},
            "live_lanes_per_wave": {"today": round(nl / max(len(waves), 1), 1), "compacted": round(nl / max(wc, 1), 1)},
            "live_runs": int(len(lens)), "live_one_off_runs": int((lens == 1).sum()),
            "live_run_length_hist": {str(k): v for k, v in sorted(hist.items())},
        }

    def size_class(x):
        for b in (512, 1024, 2048, 2730):
            if x <= b:
                return f"<={b}"
        return ">2730"

    def cbytes(t_, n_):
        return 8192 if t_ == 2 else 2 * int(n_)

    def bucket(x):
        for b in (16, 64, 256, 512, 1024, 2048, 4096):
            if x <= b:
                return b
        return 99999
    for s in range(args.sample):
        base = sb[s]
        memo = {}

        def conts(r):
            if r in memo:
                return memo[r]
            d = dense.get(int(r))
            out = {}
            if d is not None:
                lo, hi = rp[s, d], rp[s, d + 1]
                out = {int(jj[base + k]): base + k for k in range(lo, hi)}
            memo[r] = out
            return out
        for key in range(16):
            for c0 in range(0, args.batch, args.cq):
                prev = None
                hprev = {h: None for h in hot}
                run = 0
                npairs = 0
                for q in range(c0, min(args.batch, c0 + args.cq)):
                    ia, ib = conts(A[q]).get(key), conts(B[q]).get(key)
                    if ia is None or ib is None:
                        continue
                    npairs += 1
                    ta, tb = int(typ[ia]), int(typ[ib])
                    st[f"pair {('-', 'arr', 'bmp', 'run')[ta]}&{('-', 'arr', 'bmp', 'run')[tb]}"] += 1
                    if tb == 1:
                        nb_hist[bucket(int(n[ib]))] += 1
                        probes[size_class(int(n[ib]))] += int(n[ib])
                    ref_bytes += cbytes(tb, n[ib])
                    da, db = dense.get(int(A[q])), dense.get(int(B[q]))
                    for h, c in hot.items():
                        if h and da in hot_set[h] and db in hot_set[h]:
                            continue          # looked up, not counted
                        a_tw = ta == 1 and n[ia] > args.hot_twin_cutoff and da in hot_twin
                        b_tw = tb == 1 and n[ib] > args.hot_twin_cutoff and db in hot_twin
                        c["pairs"] += 1
                        if tb == 1 and not b_tw:
                            c["array_probes"] += int(n[ib])
                        if b_tw:
                            c["twin_B_pairs"] += 1
                        elif tb == 2:
                            c["bitmap_B_pairs"] += 1
                        c["referenced_bytes"] += 8192 if b_tw else cbytes(tb, n[ib])
                        if ia != hprev[h]:
                            c["stagings"] += 1
                            c["referenced_bytes"] += 8192 if a_tw else cbytes(ta, n[ia])
                            hprev[h] = ia
                    for t in cuts:
                        a_tw = ta == 1 and n[ia] > t and da in twin_rows[t]
                        b_tw = tb == 1 and n[ib] > t and db in twin_rows[t]
                        tw[t]["pairs_A_twinned"] += a_tw
                        tw[t]["pairs_B_twinned"] += b_tw
                        tw[t]["pairs_A_or_B_twinned"] += a_tw or b_tw
                        if b_tw:
                            tw[t]["probes_removed"] += int(n[ib])
                            tw[t]["extra_bytes"] += 8192 - 2 * int(n[ib])
                        if a_tw and ia != prev:
                            tw[t]["array_stagings_removed"] += 1
                            tw[t]["extra_bytes"] += 8192 - 2 * int(n[ia])
                    if ia != prev:
                        if prev is not None:
                            runlen[min(run, 64)] += 1
                        run = 0
                        st["stagings"] += 1
                        st[f"stage {('-', 'arr', 'bmp', 'run')[ta]}"] += 1
                        if ta == 1:
                            na_stage_hist[bucket(int(n[ia]))] += 1
                            stage_cls[size_class(int(n[ia]))] += 1
                        ref_bytes += cbytes(ta, n[ia])
                        prev = ia
                    run += 1
                if prev is not None:
                    runlen[min(run, 64)] += 1
                pairs_per_wave.append(npairs)
    f = 954 / args.sample
    out = {k: round(v * f) for k, v in sorted(st.items())}
    out["B_array_size_hist"] = {k: round(v * f) for k, v in sorted(nb_hist.items())}
    out["A_array_staged_size_hist"] = {k: round(v * f) for k, v in sorted(na_stage_hist.items())}
    out["B_array_probes_by_size"] = {k: round(v * f) for k, v in probes.items()}
    out["A_array_stagings_by_size"] = {k: round(v * f) for k, v in stage_cls.items()}
    out["referenced_bytes"] = round(ref_bytes * f)
    out["twin"] = {str(t): dict({k: round(int(v) * f) for k, v in sorted(tw[t].items())}, rows=len(twin_rows[t]),
                                extra_bytes_share=round(tw[t]["extra_bytes"] / max(ref_bytes, 1), 4))
                   for t in cuts}
    today = hot[0]
    out["hot_pairs"] = {str(h): dict({k: round(int(v) * f) for k, v in sorted(c.items()) if k != "queries_answered"},
                                     queries_answered_share=round(c["queries_answered"] / args.batch, 4),
                                     **{k + "_share": round(c[k] / max(today[k], 1), 4)
                                        for k in ("pairs", "array_probes", "stagings", "referenced_bytes")},
                                     bitmap_or_twin_B_pairs_share=round(
                                         (c["twin_B_pairs"] + c["bitmap_B_pairs"]) /
                                         max(today["twin_B_pairs"] + today["bitmap_B_pairs"], 1), 4))
                        for h, c in hot.items() if h}
    out["compaction"] = compaction
    rl = sorted(runlen.items())
    out["run_length_hist"] = {k: round(v * f) for k, v in rl}
    out["one_off_runs"] = round(runlen[1] * f)
    ppw = np.asarray(pairs_per_wave)
    out["pairs_per_wave"] = {"mean": float(ppw.mean()), "p50": float(np.median(ppw)), "max": int(ppw.max())}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
