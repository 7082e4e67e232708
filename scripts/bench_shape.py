#!/usr/bin/env python
"""Config 2's batch with and without the matched shape (DESIGN.md §3 rule 7f).

--leg on|off runs the batch (10k vehicles x 100 points on the config-2 graph)
--batches times, one batch at a time, with the shape's switch on or off and
nothing else.  The `on` leg makes and fetches the shape after every batch and
times the first call's three parts on the host, each ended by a wait for the
device:
  count_ms   otm_shape_size: the traversal offsets, k_shape<false>, the two
             scans and the copy of the offsets (the call's one wait), and the
             launch of k_shape<true>
  write_ms   a device synchronisation behind it: what is left of k_shape<true>
  d2h_ms     otm_fetch_shape: the copy of the three arrays
and `refetch_ms`, a second fetch (the copy alone).  Under
`rocprofv3 --kernel-trace --stats` the same run gives the two passes' kernel
times (profiles/shape/README.md).  Prints one JSON line.  Not part of bench.py.
"""
import argparse
import ctypes as C
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


def _ms(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("on", "off"), required=True)
    ap.add_argument("--batches", type=int, default=12)
    args = ap.parse_args()
    from reporter_amd import Engine, _lib
    graph, batch = config2_batch()
    hip = C.CDLL("libamdhip64.so")
    out = {"leg": args.leg, "batches": args.batches, "points": int(len(batch["lat"]))}
    with Engine(graph_path=graph, shape=args.leg == "on") as eng:
        ms, parts = [], {"count_ms": [], "write_ms": [], "d2h_ms": [], "refetch_ms": []}
        for _ in range(args.batches):
            t, res = _ms(lambda: eng.match(batch))
            ms.append(t)
            if args.leg == "on":
                z = _lib.ShapeSizes()
                parts["count_ms"].append(_ms(lambda: _lib.lib().otm_shape_size(eng.h, C.byref(z)))[0])
                parts["write_ms"].append(_ms(hip.hipDeviceSynchronize)[0])
                t, got = _ms(eng.shape)
                parts["d2h_ms"].append(t)
                parts["refetch_ms"].append(_ms(eng.shape)[0])
        out["match_ms_median"] = round(float(np.median(ms)), 3)
        out["segments"] = int(len(res.segments))
        if args.leg == "on":
            out.update({k: round(float(np.median(v)), 3) for k, v in parts.items()})
            vtx, vtx_off, spans, trav_off, poly, poly_off = got
            nt = len(vtx_off) - 1
            out["shape"] = {"traces": nt, "traversals": int(len(spans)), "vertices": int(len(vtx)),
                            "bytes": int(len(poly)), "vertices_per_trace": round(len(vtx) / nt, 2),
                            "bytes_per_trace": round(len(poly) / nt, 2),
                            "bytes_per_vertex": round(len(poly) / max(len(vtx), 1), 3),
                            "max_vertices": int(np.diff(vtx_off).max()), "max_bytes": int(np.diff(poly_off).max()),
                            "empty_traces": int((np.diff(vtx_off) == 0).sum())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
