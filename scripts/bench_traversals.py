#!/usr/bin/env python
"""Config 2's batch with and without the matched route (DESIGN.md §3 rule 7d).

--leg on|off runs the batch (10k vehicles x 100 points on the config-2 graph)
--batches times, one batch at a time, with the switch on or off and nothing
else: the two runs of a kernel trace that give k_traversals' time beside
k_seg_bound's and k_segments' (profiles/traversals/README.md).  The `on` leg
also fetches the records once (which compacts them on the device) and prints
what they hold.  Prints one JSON line.  Not part of bench.py.
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
    with Engine(graph_path=graph, traversals=args.leg == "on") as eng:
        ms = []
        for _ in range(args.batches):
            t = time.perf_counter()
            res = eng.match(batch)
            ms.append((time.perf_counter() - t) * 1e3)
        out["match_ms_median"] = round(float(np.median(ms)), 3)
        out["segments"] = int(len(res.segments))
        if args.leg == "on":
            t = time.perf_counter()
            recs, off = eng.traversals()
            out["fetch_ms"] = round((time.perf_counter() - t) * 1e3, 3)
            t = time.perf_counter()
            eng.traversals()
            out["refetch_ms"] = round((time.perf_counter() - t) * 1e3, 3)
            f = recs["flags"]
            out["records"] = {"all": int(len(recs)), "bytes": int(recs.nbytes)}
            out["records"].update({n: int(((f & b) != 0).sum()) for n, b in (
                ("chain_start", _lib.TV_CHAIN_START), ("chain_end", _lib.TV_CHAIN_END),
                ("from_start", _lib.TV_FROM_START), ("to_end", _lib.TV_TO_END), ("internal", _lib.TV_INTERNAL),
                ("segment_first", _lib.TV_SEGMENT_FIRST))})
            ids = res.segments["segment_id"][np.repeat(res.traces["seg_off"], np.diff(off)) + recs["segment"]]
            out["records"]["without_osmlr"] = int((ids < 0).sum())
            out["traces_without_records"] = int((np.diff(off) == 0).sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
