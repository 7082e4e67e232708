#!/usr/bin/env python
"""The pair window's flush on the GPU against the Python definition.

Two shapes, each timed from the call to the body's bytes on the host:
  config2  the window of one config-2 bench batch (10k vehicles x 100 points,
           one-minute buckets) on the real config-2 graph, filled by the match
           (untimed) and closed by Engine.pairs_flush (timed);
  keys     --keys distinct keys (default 2^20) filled through
           Engine.pairs_add_reports (its own time reported) and flushed.
Median and range over --repeats after --warm warm runs; the Python definition
(datastore.serialize(datastore.pair_records(...))) on the same reports in the
same process, and the bodies compared once per shape.
--leg on|off runs config 2's batch --batches times, one batch at a time, with
or without a pair window and nothing else: the two runs of a kernel trace
that give the report kernel's time with and without the upsert
(profiles/pairs/README.md).
Writes one JSON file (--out) and prints it.  Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUCKET_S, ORIGIN = 60, 1499999940


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4),
            "runs": len(xs)}


def python_path(reports, ids, reps):
    from reporter_amd import datastore
    out, body, st = [], None, None
    for _ in range(reps):
        t = time.perf_counter()
        d, st = datastore.pair_records(reports, ids, BUCKET_S, ORIGIN, 1)
        body = datastore.serialize(d)
        out.append((time.perf_counter() - t) * 1e3)
    return body, st, stats(out)


def config2_batch():
    from reporter_amd import synth
    graph = synth.cached_graph(2)
    t = synth.CONFIGS[2]["traces"]
    return graph, synth.make_traces(graph, t["n_vehicles"], t["points_per_vehicle"], interval_s=t["interval_s"],
                                    noise_sigma_m=t["noise_sigma_m"], accuracy=t["accuracy"], seed=7)


def key_records(n, ids):
    """n records on n distinct keys (bucket, row, next row)."""
    from reporter_amd import _lib
    j = np.arange(n, dtype=np.int64)
    gi, k = j // 4096, j % 4096
    if gi.max() >= len(ids):
        raise SystemExit("--keys needs %d segments, the graph has %d" % (gi.max() + 1, len(ids)))
    sid = np.asarray(ids).astype(np.uint64).view(np.int64)
    rec = np.zeros(n, _lib.REPORT_DTYPE)
    rec["id"] = sid[gi]
    rec["next_id"] = sid[(gi + 1 + j % 7) % len(ids)]
    rec["t0"] = ORIGIN + k * BUCKET_S + (j % 50) + 0.25
    rec["t1"] = rec["t0"] + 1.0 + (j % 7) * 0.5
    rec["length"] = 10 + gi
    rec["queue_length"] = j % 5
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--leg", choices=("on", "off"), default=None, help="only config 2's batches, for a kernel trace")
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "bench_pairs.json"))
    args = ap.parse_args()
    import torch

    from reporter_amd import Engine, _lib, synth
    graph, batch = config2_batch()
    if args.leg:
        with Engine(graph_path=graph) as eng:
            if args.leg == "on":
                eng.pairs_begin(BUCKET_S, ORIGIN)
            for _ in range(args.batches):
                res = eng.match(batch)
            if args.leg == "on":
                _, st = eng.pairs_flush()
                eng.pairs_end()
                print(json.dumps({"leg": "on", "batches": args.batches, "reports_per_batch": len(res.reports),
                                  "stats": st}))
            else:
                print(json.dumps({"leg": "off", "batches": args.batches, "reports_per_batch": len(res.reports)}))
        return
    ids = synth.segment_ids(graph)
    res = {"device": torch.cuda.get_device_name(0), "hip_runtime": _lib.runtime_info(), "torch": torch.__version__,
           "library": os.path.relpath(_lib.LIB_PATH, ROOT), "repeats": args.repeats, "warm": args.warm,
           "bucket_s": BUCKET_S, "origin": ORIGIN, "privacy": 1}
    with Engine(graph_path=graph) as eng:
        # ---- config 2: the window of one bench batch
        eng.pairs_begin(BUCKET_S, ORIGIN)
        info = eng.pairs_info()
        ts, body, st, reports = [], None, None, None
        for k in range(args.warm + args.repeats):
            reports = eng.match(batch).reports.copy()
            t0 = time.perf_counter()
            body, st = eng.pairs_flush()
            if k >= args.warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        eng.pairs_end()
        want, wst, py = python_path(reports, ids, 5)
        res["config2"] = {"segments": len(ids), "reports": len(reports), "stats": st, "table": info,
                          "body_bytes": len(body), "bytes_equal": body == want and st == wst, "pairs_flush": stats(ts),
                          "python_path": py, "speedup_median": round(py["median_ms"] / stats(ts)["median_ms"], 1)}
        print(json.dumps({"config2": res["config2"]}), flush=True)
        # ---- --keys distinct keys through otm_pairs_add_reports
        rec = key_records(args.keys, ids)
        eng.pairs_begin(BUCKET_S, ORIGIN, max_keys=args.keys)
        info = eng.pairs_info()
        ts, fill = [], []
        for k in range(args.warm + args.repeats):
            t0 = time.perf_counter()
            eng.pairs_add_reports(rec)
            t1 = time.perf_counter()
            body, st = eng.pairs_flush()
            if k >= args.warm:
                fill.append((t1 - t0) * 1e3)
                ts.append((time.perf_counter() - t1) * 1e3)
        eng.pairs_end()
        want, wst, py = python_path(rec, ids, 3)
        res["keys"] = {"keys": args.keys, "stats": st, "table": info, "body_bytes": len(body),
                       "bytes_equal": body == want and st == wst, "pairs_add_reports": stats(fill),
                       "pairs_flush": stats(ts), "python_path": py,
                       "speedup_median": round(py["median_ms"] / stats(ts)["median_ms"], 1)}
        print(json.dumps({"keys": res["keys"]}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
