#!/usr/bin/env python
"""Config 2's batch with and without matched points (DESIGN.md §3 rule 7c).

--leg on|off runs the batch (10k vehicles x 100 points on the config-2 graph)
--batches times, one batch at a time, with the switch on or off and nothing
else: the two runs of a kernel trace that give k_points' time beside its
neighbours' (profiles/points/README.md).  The `on` leg also fetches the
records once and prints what they hold.  Prints one JSON line.  Not part of
bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def config2_batch():
    from reporter_amd import synth
    graph = synth.cached_graph(2)
    t = synth.CONFIGS[2]["traces"]
    return graph, synth.make_traces(graph, t["n_vehicles"], t["points_per_vehicle"], interval_s=t["interval_s"],
                                    noise_sigma_m=t["noise_sigma_m"], accuracy=t["accuracy"], seed=7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("on", "off"), required=True)
    ap.add_argument("--batches", type=int, default=12)
    args = ap.parse_args()
    from reporter_amd import Engine, _lib
    graph, batch = config2_batch()
    out = {"leg": args.leg, "batches": args.batches, "points": int(len(batch["lat"]))}
    with Engine(graph_path=graph, matched_points=args.leg == "on") as eng:
        ms = []
        for _ in range(args.batches):
            t = time.perf_counter()
            res = eng.match(batch)
            ms.append((time.perf_counter() - t) * 1e3)
        out["match_ms_median"] = round(float(np.median(ms)), 3)
        out["segments"] = int(len(res.segments))
        if args.leg == "on":
            t = time.perf_counter()
            pts = eng.points()
            out["fetch_ms"] = round((time.perf_counter() - t) * 1e3, 3)
            f = pts["flags"]
            out["records"] = {n: int(((f & b) != 0).sum()) for n, b in (
                ("matched", _lib.PT_MATCHED), ("column", _lib.PT_COLUMN), ("node", _lib.PT_NODE),
                ("route", _lib.PT_ROUTE), ("anchor", _lib.PT_ANCHOR), ("same_edge", _lib.PT_SAME_EDGE))}
            m = (f & _lib.PT_MATCHED) != 0
            d = pts["distance"][m]
            out["distance_m"] = {"median": round(float(np.median(d)), 2), "p99": round(float(np.percentile(d, 99)), 2),
                                 "max": round(float(d.max()), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
